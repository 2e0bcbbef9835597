"""The recent-items recommender without a GPU: the numpy mirror of its rule (tests/recent_items_emulation.py) against brute
force on a table whose dot products are exact, the mirror's history rule at its edges, the validation of
pinsage.evaluation.RecentItemsRecommender, and the argument checks of mi_recent_items / mi_pool_recent_f32 /
mi_topk_merge_max_f32 (they return before anything touches a device)."""
import numpy as np
import pytest

import recent_items_emulation as RE
from laplace_amd.pinsage.evaluation import RecentItemsRecommender

N_ITEMS, K = 300, 10


@pytest.fixture(scope="module")
def data():
    h = RE.dyadic_table(N_ITEMS, 16, seed=1)
    rows = RE.history_rows(N_ITEMS, 8, seed=2)
    rng = np.random.default_rng(3)
    rows.append(rng.permutation(N_ITEMS)[:N_ITEMS - 3].tolist() + [5, 5])      # 3 or 4 items left: fewer than K
    return h, rows


def test_table_is_exact(data):
    h, _ = data
    assert h.shape == (N_ITEMS, 16) and h.any(axis=1).all()
    assert np.array_equal(h * 4, np.round(h * 4)) and np.abs(h).max() <= 2
    full = h.astype(np.float64) @ h.astype(np.float64).T
    assert np.array_equal(RE.scores_fma(h, h).astype(np.float64), full)       # the fma chain gives the exact products


@pytest.mark.parametrize("n_recent", [1, 2, 8, 16])
def test_max_with_decay_one_is_the_top_k_of_the_max_score(data, n_recent):
    """The claim of the rule: anything that outranks item i in its arg-max slot's list also outranks it in the result, so
    merging per-slot top-K lists loses nothing."""
    h, rows = data
    ids, sc = RE.recommend(rows, h, n_recent, "max", 1.0, K)
    want_ids, want_sc = RE.brute_force_max(rows, h, n_recent, K)
    assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc)
    assert (ids[-1] >= 0).sum() in (3, 4) and (ids[-1][4:] == -1).all() and np.isneginf(sc[-1][4:]).all()


def test_max_with_decay_half_is_the_procedure(data):
    """decay = 0.5: the weights are powers of two, the products stay exact; against the definition written out per user."""
    h, rows = data
    n_recent = 8
    ids, sc = RE.recommend(rows, h, n_recent, "max", 0.5, K)
    full = h.astype(np.float64) @ h.astype(np.float64).T
    differs = 0
    for u, row in enumerate(rows):
        slots = RE.history(row, n_recent)
        allowed = np.setdiff1d(np.arange(N_ITEMS), row)
        cand = {}
        for r, item in enumerate(slots):
            s = full[item, allowed]
            top = allowed[np.lexsort((allowed, -s))][:K]                       # slot r's own list
            for i in top:
                cand[int(i)] = max(cand.get(int(i), -np.inf), 0.5 ** r * full[item, i] + 0.0)
        order = sorted(cand.items(), key=lambda kv: (-kv[1], kv[0]))[:K]
        n = len(order)
        assert ids[u, :n].tolist() == [i for i, _ in order] and (ids[u, n:] == -1).all(), u
        assert sc[u, :n].tolist() == [s for _, s in order] and np.isneginf(sc[u, n:]).all(), u
        # and it is NOT the closed form any more: an item outside slot r's top-K can beat what the lists hold
        closed = np.max([0.5 ** r * full[item] for r, item in enumerate(slots)], axis=0)
        best = allowed[np.lexsort((allowed, -closed[allowed]))][:K]
        differs += best.tolist() != ids[u, :n].tolist()
    print("users whose decay = 0.5 answer differs from the closed form:", differs)


def test_n_recent_one_is_the_latest_item(data):
    h, rows = data
    full = RE.scores_fma(h, h)
    latest = np.array([r[-1] for r in rows])
    want = RE.topk_excl(full[latest], rows, K)
    for pool in ("max", "mean"):
        got = RE.recommend(rows, h, 1, pool, 0.7, K)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), pool


@pytest.mark.parametrize("n_recent", [1, 3, 8, 16])
def test_history_rule(n_recent):
    rows = RE.history_rows(N_ITEMS, n_recent, seed=4)
    assert [len(r) for r in rows[:6]] == [1, n_recent, 63, 64, 65, 300]
    items, n_slots = RE.recent_items(rows, n_recent)
    assert items.shape == (n_recent, len(rows)) and items.dtype == np.int64 and n_slots.dtype == np.int32
    for u, row in enumerate(rows):
        window = row[-64:]
        distinct = list(dict.fromkeys(reversed(window)))                       # most recent occurrence first
        ns = int(n_slots[u])
        assert ns == min(len(distinct), n_recent) >= 1
        assert items[:ns, u].tolist() == distinct[:ns] and items[0, u] == row[-1]
        assert (items[ns:, u] == row[-1]).all()                                # unused slots: the slot-0 item
    one, all_distinct, seventeenth, before, again = 6, 7, 8, 9, 10
    assert n_slots[one] == 1
    assert n_slots[all_distinct] == n_recent and items[:, all_distinct].tolist() == rows[all_distinct][::-1][:n_recent]
    assert len(set(rows[seventeenth])) == 17 and rows[seventeenth][0] not in items[:, seventeenth]
    assert n_slots[seventeenth] == min(16, n_recent)
    assert len(set(rows[before])) == 12 and n_slots[before] == min(len(set(rows[before][-64:])), n_recent) <= 5
    assert n_slots[again] == min(2, n_recent) and items[0, again] == rows[again][-1]
    with pytest.raises(ValueError):
        RE.recent_items(rows + [[]], n_recent)


def test_weights_and_mean_chain():
    w = RE.weights(0.9, 8)
    assert w.dtype == np.float32 and w[0] == 1.0 and w[3] == np.float32(0.9 ** 3)
    assert RE.weights(1.0, 16).tolist() == [1.0] * 16
    h = np.random.default_rng(0).standard_normal((20, 8)).astype(np.float32)
    items = np.array([[3, 4], [5, 4], [7, 4]], dtype=np.int64)                # user 1 has one slot, its fill repeats item 4
    q = RE.pool_mean(items, np.array([3, 1], dtype=np.int32), w[:3], h)
    assert np.array_equal(q[1], h[4])                                          # (1 * h) / 1
    acc = (np.float32(1) * h[3]) + np.float32(0)
    acc = acc + w[1] * h[5]
    acc = acc + w[2] * h[7]
    assert np.array_equal(q[0], acc / np.float32(np.float32(np.float32(1) + w[1]) + w[2]))
    assert abs(q[0] - (h[3] + 0.9 * h[5] + 0.81 * h[7]) / 2.71).max() < 1e-6


def test_recommender_validates():
    r = RecentItemsRecommender()
    assert (r.n_recent, r.pool, r.decay) == (8, "max", 1.0)
    assert np.array_equal(RecentItemsRecommender(5, "mean", 0.9).weights(), RE.weights(0.9, 5))
    for bad in (dict(n_recent=0), dict(n_recent=17), dict(n_recent=-1), dict(n_recent=2.5), dict(pool="sum"), dict(pool=None),
                dict(decay=0.0), dict(decay=1.01), dict(decay=-0.5), dict(decay=float("nan"))):
        with pytest.raises(ValueError):
            RecentItemsRecommender(**bad)


def test_c_entries_validate_before_anything_is_enqueued():
    from laplace_amd import _lib
    L = _lib.lib()
    fake = 4096
    BAD, UNS = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_UNSUPPORTED

    def recent(n_users=8, n_recent=8, ptr=fake, idx=fake, items=fake, slots=fake):
        return L.mi_recent_items(n_users, ptr, idx, n_recent, items, slots, None)

    def pool(n_users=8, n_recent=8, d=16, items=fake, slots=fake, w=fake, table=fake, ld=16, q=fake, ldq=16):
        return L.mi_pool_recent_f32(n_users, n_recent, d, items, slots, w, table, ld, q, ldq, None)

    def merge(n_q=8, n_lists=8, k_in=12, k_out=12, ids=fake, sc=fake, slots=fake, w=fake, out=fake, out_sc=fake):
        return L.mi_topk_merge_max_f32(n_q, n_lists, k_in, k_out, ids, sc, slots, w, out, out_sc, None)

    assert recent(n_recent=0) == BAD and recent(n_recent=-3) == BAD and recent(n_recent=17) == UNS
    assert recent(n_users=-1) == BAD and recent(n_users=1 << 31) == _lib.MI_ERR_TOO_LARGE
    for null in ("ptr", "idx", "items", "slots"):
        assert recent(**{null: None}) == BAD, null
    assert recent(items=fake + 4) == BAD                                       # int64 output, 4-byte aligned
    assert recent(n_users=0, ptr=None, idx=None, items=None, slots=None) == 0  # nothing to do, nothing enqueued

    assert pool(n_recent=0) == BAD and pool(n_recent=17) == UNS
    for d in (1, 2, 3, 5, 18):
        assert pool(d=d, ld=20, ldq=20) == UNS, d
    assert pool(d=0) == BAD and pool(n_users=-1) == BAD
    assert pool(ld=12) == BAD and pool(ldq=12) == BAD and pool(ld=18) == BAD and pool(ldq=17) == BAD
    assert pool(table=fake + 4) == BAD and pool(q=fake + 8) == BAD
    for null in ("items", "slots", "w", "table", "q"):
        assert pool(**{null: None}) == BAD, null
    assert pool(n_users=0) == 0

    assert merge(n_lists=17, k_in=241) == UNS                                  # 4097 entries
    assert merge(n_lists=1, k_in=4097, k_out=10) == UNS
    assert merge(n_lists=1 << 16, k_in=1 << 16, k_out=1) == UNS                # the product does not wrap
    assert merge(k_in=12, k_out=13) == BAD
    assert merge(n_lists=0) == BAD and merge(k_in=0, k_out=0) == BAD and merge(k_out=0) == BAD and merge(n_q=-1) == BAD
    for null in ("ids", "sc", "slots", "w", "out"):
        assert merge(**{null: None}) == BAD, null
    assert merge(ids=fake + 4) == BAD and merge(out_sc=fake + 2) == BAD
    assert merge(n_q=0) == 0
