"""GPU: the recent-items recommender (N5) — mi_recent_items, mi_pool_recent_f32 and mi_topk_merge_max_f32 each against the numpy
mirror of the rule (tests/recent_items_emulation.py), RecentItemsRecommender end to end against the mirror and, where the rule
has a closed form, against brute force; its n_recent = 1 case against LatestNNRecommender; evaluate_nn's default; a planted
case in which only the second-latest item leads to the held-out one; and calls that follow other calls.  Everything is bit for
bit."""
import numpy as np
import pytest
import torch as t

import recent_items_emulation as RE
from laplace_amd.pinsage.evaluation import LatestNNRecommender, RecentItemsRecommender, evaluate_nn, prec

pytestmark = pytest.mark.gpu

N_ITEMS, K = 300, 10


def _dev(a):
    return t.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(rows):
    ptr, idx = RE.csr_of(rows)
    return _dev(ptr), _dev(idx)


def _few_left(n_items, seed=3):
    """A row that leaves 3 items (and repeats one of its own): fewer than K eligible."""
    return np.random.default_rng(seed).permutation(n_items)[:n_items - 3].tolist() + [5, 5]


@pytest.fixture(scope="module")
def small():
    """300 items (top-K's materialised path), the history rule's edge rows, one user with fewer than K eligible items."""
    h = RE.dyadic_table(N_ITEMS, 16, seed=1)
    rows = RE.history_rows(N_ITEMS, 8, seed=2) + [_few_left(N_ITEMS)]
    return h, rows, _dev(h), _graph(rows)


# ---- the three kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_recent", [1, 3, 8, 16])
def test_recent_items_kernel(n_recent):
    from laplace_amd import ops
    rows = RE.history_rows(N_ITEMS, n_recent, seed=4)
    assert 38 <= len(rows) <= 45 and [len(r) for r in rows[:6]] == [1, n_recent, 63, 64, 65, 300]
    ptr, idx = _graph(rows)
    items, n_slots = ops.recent_items(ptr, idx, n_recent)
    want_items, want_slots = RE.recent_items(rows, n_recent)
    assert items.dtype == t.int64 and n_slots.dtype == t.int32
    assert np.array_equal(items.cpu().numpy(), want_items) and np.array_equal(n_slots.cpu().numpy(), want_slots)
    again = ops.recent_items(ptr, idx, n_recent)
    assert t.equal(again[0], items) and t.equal(again[1], n_slots)
    got = RecentItemsRecommender(n_recent).recent_items((ptr, idx), device="cuda")
    assert t.equal(got[0], items) and t.equal(got[1], n_slots)


@pytest.mark.parametrize("d", [4, 16, 128])
@pytest.mark.parametrize("n_recent", [8, 16])
def test_pool_kernel(d, n_recent):
    from laplace_amd import ops
    rows = RE.history_rows(N_ITEMS, n_recent, seed=5)
    items, n_slots = RE.recent_items(rows, n_recent)
    assert (n_slots == 1).any() and (n_slots == n_recent).any() and ((n_slots > 1) & (n_slots < n_recent)).any()
    h = np.random.default_rng(d).standard_normal((N_ITEMS, d)).astype(np.float32)
    for decay in (1.0, 0.9):
        w = RE.weights(decay, n_recent)
        q = ops.pool_recent(_dev(items), _dev(n_slots), _dev(w), _dev(h))
        want = RE.pool_mean(items, n_slots, w, h)
        assert q.shape == (len(rows), d) and np.array_equal(q.cpu().numpy().view(np.uint32), want.view(np.uint32)), decay
    wide = t.full((N_ITEMS, d + 4), float("nan"), device="cuda")                 # a row-strided table: ld = d + 4
    wide[:, :d] = _dev(h)
    assert t.equal(ops.pool_recent(_dev(items), _dev(n_slots), _dev(w), wide[:, :d]), q)


def _lists(n_lists, n_q, k_in, seed):
    """Handed-in lists: ids from a catalogue of 2 * k_in + 3 items (the same id in several lists), scores partly on a coarse
    grid (equal scores across ids), zeros of each sign, -1 pads inside the lists, n_slots anywhere in 0 .. n_lists."""
    rng = np.random.default_rng(seed)
    n_items = 2 * k_in + 3
    ids = np.stack([np.stack([rng.permutation(n_items)[:k_in] for _ in range(n_q)]) for _ in range(n_lists)]).astype(np.int64)
    sc = rng.standard_normal((n_lists, n_q, k_in)).astype(np.float32)
    grid = rng.random(sc.shape) < 0.4
    sc[grid] = np.round(sc[grid] * 2) / 2                                        # multiples of 1/2, 0 and -0 among them
    sc[rng.random(sc.shape) < 0.05] = np.float32(0.0)
    sc[rng.random(sc.shape) < 0.05] = np.float32(-0.0)
    pad = rng.random(sc.shape) < 0.1
    ids[pad], sc[pad] = -1, -np.inf
    # planted in every query's first list: a zero of each sign, one score on two ids, a pad before the list's end; and list 1
    # repeats an id of list 0
    ids[0, :, :4] = np.stack([rng.permutation(n_items)[:4] for _ in range(n_q)])
    sc[0, :, 0], sc[0, :, 1], sc[0, :, 2], sc[0, :, 3] = np.float32(0.0), np.float32(-0.0), np.float32(0.5), np.float32(0.5)
    ids[0, :, 4], sc[0, :, 4] = -1, -np.inf
    if n_lists > 1:
        ids[1, :, 0], sc[1, :, 0] = ids[0, :, 1], np.float32(-0.0)
    n_slots = rng.integers(1, n_lists + 1, n_q).astype(np.int32)
    n_slots[0] = n_lists
    if n_q > 2:
        n_slots[1], n_slots[2] = 1, 0
    assert np.signbit(sc[sc == 0]).any() and not np.signbit(sc[sc == 0]).all()
    return ids, sc, n_slots


@pytest.mark.parametrize("n_q", [1, 65, 300])
@pytest.mark.parametrize("shape", [(1, 12, 12), (8, 12, 12), (3, 5, 5), (16, 256, 256), (16, 256, 10)], ids=str)
def test_merge_kernel(shape, n_q):
    from laplace_amd import ops
    n_lists, k_in, k_out = shape
    ids, sc, n_slots = _lists(n_lists, n_q, k_in, seed=n_lists * 1000 + k_in + n_q)
    for decay in (1.0, 0.9):
        w = RE.weights(decay, n_lists)
        args = (_dev(ids), _dev(sc), _dev(n_slots), _dev(w), k_out)
        out_ids, out_sc = ops.topk_merge_max(*args)
        want_ids, want_sc = RE.merge_max(ids, sc, n_slots, w, k_out)
        assert np.array_equal(out_ids.cpu().numpy(), want_ids), decay
        assert np.array_equal(out_sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32)), decay   # +0 for every zero
        again = ops.topk_merge_max(*args)
        assert t.equal(again[0], out_ids) and t.equal(again[1].view(t.int32), out_sc.view(t.int32))
        assert t.equal(ops.topk_merge_max(*args, want_scores=False), out_ids)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from laplace_amd import _lib, ops
    ptr, idx = t.tensor([0, 2], dtype=t.int32), t.tensor([1, 2], dtype=t.int32)
    with pytest.raises(_lib.MiError):
        ops.recent_items(ptr, idx, 4)
    with pytest.raises(_lib.MiError):
        RecentItemsRecommender(4).recent_items((ptr, idx))
    items, n_slots, w = t.zeros(2, 1, dtype=t.int64), t.ones(1, dtype=t.int32), t.ones(2)
    with pytest.raises(_lib.MiError):
        ops.pool_recent(items, n_slots, w, t.zeros(3, 4))
    with pytest.raises(_lib.MiError):
        ops.topk_merge_max(t.zeros(2, 1, 3, dtype=t.int64), t.zeros(2, 1, 3), n_slots, w, 3)
    with pytest.raises(_lib.MiError, match="-4"):                                # d % 4 != 0: MI_ERR_UNSUPPORTED
        ops.pool_recent(items.cuda(), n_slots.cuda(), w.cuda(), t.zeros(3, 6, device="cuda"))
    with pytest.raises(ValueError):
        ops.pool_recent(items.cuda(), n_slots.cuda(), t.ones(3, device="cuda"), t.zeros(3, 4, device="cuda"))
    with pytest.raises(ValueError):
        RecentItemsRecommender(16).recommend((ptr.cuda(), idx.cuda()), 257, None, t.zeros(300, 4, device="cuda"))   # 4112 entries


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _same(got, want):
    ids, sc = got
    return np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(sc.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("decay", [1.0, 0.5])
@pytest.mark.parametrize("n_recent", [2, 8])
def test_recommend_small_catalogue(small, pool, decay, n_recent):
    from laplace_amd import _lib, ops
    h, rows, h_dev, graph = small
    assert ops.topk_path(h_dev, h_dev, K) == _lib.MI_TOPK_PATH_MATERIALISED
    rec = RecentItemsRecommender(n_recent, pool, decay)
    got = rec.recommend(graph, K, None, h_dev, want_scores=True)
    assert got[0].shape == (len(rows), K) and got[0].dtype == t.int64 and got[1].dtype == t.float32
    assert _same(got, RE.recommend(rows, h, n_recent, pool, decay, K))
    if pool == "max" and decay == 1.0:
        assert _same(got, RE.brute_force_max(rows, h, n_recent, K))
    assert t.equal(rec.recommend(graph, K, None, h_dev), got[0])
    last = got[0][-1].cpu()                                                       # the user with 3 or 4 items left
    n_left = N_ITEMS - len(set(rows[-1]))
    assert n_left < K and bool((last[:n_left] >= 0).all()) and bool((last[n_left:] == -1).all())
    assert bool(t.isneginf(got[1][-1, n_left:]).all())


def test_recommend_fused_path_catalogue():
    """32 768 items at d = 16: every slot's top-K is served by the fused kernel."""
    from laplace_amd import _lib, ops
    n_items = 32_768
    h = RE.dyadic_table(n_items, 16, seed=6)
    rows = RE.history_rows(n_items, 8, seed=7, n_random=53)
    assert len(rows) == 64
    h_dev, graph = _dev(h), _graph(rows)
    assert ops.topk_path(h_dev, h_dev, K) == _lib.MI_TOPK_PATH_FUSED
    for pool, decay in (("max", 0.5), ("mean", 1.0)):
        got = RecentItemsRecommender(8, pool, decay).recommend(graph, K, None, h_dev, want_scores=True)
        assert _same(got, RE.recommend(rows, h, 8, pool, decay, K)), pool


def test_chunked_users_equal_one_chunk(small, monkeypatch):
    h, rows, h_dev, graph = small
    rec = RecentItemsRecommender(8, "max", 0.5)
    whole = rec.recommend(graph, K, None, h_dev, want_scores=True)
    monkeypatch.setattr(RecentItemsRecommender, "MAX_LIST_BYTES", 8 * K * 12 * 16)      # 16 users per chunk, the last one partial
    cut = rec.recommend(graph, K, None, h_dev, want_scores=True)
    assert len(rows) % 16 != 0 and t.equal(cut[0], whole[0]) and t.equal(cut[1].view(t.int32), whole[1].view(t.int32))


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_one_slot_is_the_latest_item_recommender(small, pool):
    h, rows, h_dev, graph = small
    g = t.Generator().manual_seed(9)
    for table in (h_dev, t.randn(N_ITEMS, 16, generator=g).cuda()):
        want = LatestNNRecommender().recommend(graph, K, None, table)
        for decay in (1.0, 0.7):
            assert t.equal(RecentItemsRecommender(1, pool, decay).recommend(graph, K, None, table), want), decay
    with pytest.raises(ValueError):
        RecentItemsRecommender(1, pool).recommend(_graph(rows + [[]]), K, None, h_dev)
    with pytest.raises(ValueError):
        RecentItemsRecommender(1, pool).recommend(graph, 0, None, h_dev)


def test_evaluate_nn_default_is_the_latest_item_path():
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.sampler import PinSAGESampler
    rng = np.random.default_rng(11)
    U, I = 400, 200
    u, a = rng.integers(0, U, 6000), rng.integers(0, I, 6000)
    u, a = np.r_[u, np.arange(U)], np.r_[a, rng.integers(0, I, U)]                # every user has an interaction
    users, items = AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, I)
    held = AdjList.from_edges(np.arange(U), rng.integers(0, I, U), U)
    smp = PinSAGESampler(users, items, U, I, batch_size=32, seed=3)
    t.manual_seed(0)
    model = PinSAGEModel(I, 16, 2).to("cuda")
    gt = (held.ptr, held.idx)
    today = prec(LatestNNRecommender().recommend(smp, K, None, model.item_representations(smp, step=0)), gt)
    assert evaluate_nn(model, smp, gt, K, step=0) == today
    assert evaluate_nn(model, smp, gt, K, step=0, recommender=None) == today
    assert evaluate_nn(model, smp, gt, K, step=0, recommender=RecentItemsRecommender(1, "mean")) == today
    assert evaluate_nn(model, smp, gt, K, graph=(users.ptr, users.idx), step=0, recommender=LatestNNRecommender()) == today
    recs = RecentItemsRecommender(4, "max").recommend(smp, K, None, model.item_representations(smp, step=0))
    assert evaluate_nn(model, smp, gt, K, step=0, recommender=RecentItemsRecommender(4, "max")) == prec(recs, gt)


def test_the_second_interest_is_served():
    """40 communities of 4 items; h = the community's one-hot + 1/8 at coordinate (community + 1 + place in community) % 40.
    Two items of one community score >= 1; items of different communities at most 1/8 + 1/8 + 1/64.  A user's row is
    [b, a] with a in community c and b in community c + 20, the held-out item is another item of c + 20: it scores 0 against a
    (its two coordinates c + 20 and c + 21 + place are not among a's c and c + 1 + place, places being 0 .. 3), while eight items
    score 1/8 or more against a (the four of community c + 1 + place(a), and one in each of the communities c - 1 .. c - 4), so
    the latest item's ten are the 3 others of c and 7 of those eight: never the held-out item.  With two slots, b's list
    holds the 3 others of c + 20 at scores >= 1, and at most 6 items score >= 1 in the merge: the held-out item is among the
    ten of every user."""
    C, M = 40, 4
    n_items = C * M
    h = np.zeros((n_items, C), dtype=np.float32)
    for i in range(n_items):
        c, j = divmod(i, M)
        h[i, c] = 1.0
        h[i, (c + 1 + j) % C] += 0.125
    rng = np.random.default_rng(13)
    rows, held = [], []
    for u in range(200):
        c = u % C
        a = c * M + int(rng.integers(0, M))
        jb, jh = rng.permutation(M)[:2]
        cb = (c + 20) % C
        rows.append([cb * M + int(jb), a])
        held.append(cb * M + int(jh))
    graph = _graph(rows)
    gt = (np.arange(201, dtype=np.int32), np.array(held, dtype=np.int32))
    h_dev = _dev(h)
    two = prec(RecentItemsRecommender(2, "max").recommend(graph, K, None, h_dev), gt)
    one = prec(LatestNNRecommender().recommend(graph, K, None, h_dev), gt)
    assert two == 1.0 and one == 0.0


def test_state_that_outlives_a_call(small):
    h, rows, h_dev, graph = small
    rows2 = RE.history_rows(N_ITEMS, 8, seed=21, n_random=70)
    graph2 = _graph(rows2)
    for pool in ("max", "mean"):
        rec = RecentItemsRecommender(8, pool, 0.9)
        fresh = lambda g, k: RecentItemsRecommender(8, pool, 0.9).recommend(g, k, None, h_dev, want_scores=True)
        same = lambda x, y: t.equal(x[0], y[0]) and t.equal(x[1].view(t.int32), y[1].view(t.int32))
        first = rec.recommend(graph, K, None, h_dev, want_scores=True)
        assert same(rec.recommend(graph, K, None, h_dev, want_scores=True), first)
        assert same(rec.recommend(graph, 17, None, h_dev, want_scores=True), fresh(graph, 17))
        assert same(rec.recommend(graph2, K, None, h_dev, want_scores=True), fresh(graph2, K))
        assert same(rec.recommend(graph, K, None, h_dev, want_scores=True), first)
        assert same(first, fresh(graph, K))
