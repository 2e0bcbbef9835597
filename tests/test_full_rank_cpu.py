"""CPU: the host side of the full-rank feature.  (1) mi_rank_path — the function the dispatcher of mi_rank_items_f32 itself
calls, host-only — answers every case of tests/rank_cases.py with the path the case declares, from made-up addresses with the
case's alignment, and the table covers what it was written to cover.  (2) utils.metrics_lightgcn.full_rank_metrics, pure torch
on a rank vector, against the per-user loops of tests/full_rank_reference.py: integers equal, floats within 1e-12 (both sides
are float64); against rank_metrics on the hit matrix of the reference's own top-K lists; and against a hand-computed example."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch as t

from oracle import lightgcn_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asan_driver import BAD_ARG, L, _lib  # noqa: E402
import full_rank_reference as FR  # noqa: E402
import rank_cases as C  # noqa: E402

USER_BASE, ITEM_BASE = 0x7F00_0000_0000, 0x7F40_0000_0000    # 256-byte aligned, as the caching allocator's blocks are


# ---- (1) the path rule and the table ------------------------------------------------------------------------------------------
def test_the_constants_of_the_table_are_the_bindings():
    assert (C.M, C.F) == (_lib.MI_RANK_PATH_MATERIALISED, _lib.MI_RANK_PATH_FUSED)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_every_case_takes_its_declared_path(case):
    c = case
    assert c.layout in C.T.LAYOUTS and c.excl in C.T.EXCLS and c.values in C.T.VALUES and c.uid in C.T.UIDS
    assert c.n_items <= 40_002 and c.n_q <= 257
    up, ldu, ip, ldi = C.layout_of(c, USER_BASE, ITEM_BASE)
    got = int(L.mi_rank_path(c.n_items, c.d, up, ldu, ip, ldi))
    assert got == c.path, (c.name, C.PATH_NAMES.get(got, got), C.PATH_NAMES[c.path])


def test_the_rule_itself_at_its_edges():
    a, b = USER_BASE, ITEM_BASE
    path = lambda n, d, up=a, ldu=None, ip=b, ldi=None: int(L.mi_rank_path(n, d, up, ldu or d, ip, ldi or d))
    assert path(1, 4) == C.F and path(0, 4) == C.F and path(100_000, 128) == C.F          # any catalogue size
    assert path(1_000, 132) == C.M and path(1_000, 128) == C.F and path(1_000, 126) == C.M and path(1_000, 1) == C.M
    assert path(1_000, 32, ldu=33) == C.M and path(1_000, 32, ldi=33) == C.M and path(1_000, 32, ldu=36, ldi=40) == C.F
    for off in (4, 8, 12):
        assert path(1_000, 32, up=a + off) == C.M and path(1_000, 32, ip=b + off) == C.M
    assert path(1_000, 32, up=a + 16, ip=b + 48) == C.F
    assert path(-1, 64) == BAD_ARG and path(100, 0) == BAD_ARG
    assert path(100, 64, up=None) == BAD_ARG and path(100, 64, ip=None) == BAD_ARG
    assert path(100, 64, ldu=63) == BAD_ARG and path(100, 64, ldi=63) == BAD_ARG
    assert path(2 ** 31 - 1, 64) == _lib.MI_ERR_TOO_LARGE


def test_the_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal comes before anything is enqueued."""
    n_q, n_items, d = 10, 100, 8
    need = int(L.mi_rank_items_workspace_bytes(n_q, n_items))
    assert need >= n_q * n_items * 4 + n_q * ((n_items + 31) // 32) * 4 + 2 * n_q * 4
    assert int(L.mi_rank_items_workspace_bytes(0, 100)) == 256
    p = USER_BASE
    call = lambda **kw: int(L.mi_rank_items_f32(*[kw.get(k, v) for k, v in (
        ("n_q", n_q), ("n_items", n_items), ("d", d), ("uid", p), ("target", p), ("ue", p), ("ldu", d), ("ie", p), ("ldi", d),
        ("ep", None), ("ei", None), ("rank", p), ("score", None), ("nex", None), ("ws", p), ("ws_bytes", need), ("stream", None))]))
    assert call(n_q=0) == 0
    assert call(n_q=-1) == BAD_ARG and call(n_items=-1) == BAD_ARG and call(d=0) == BAD_ARG
    for name in ("uid", "target", "ue", "ie", "rank", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(ldu=d - 1) == BAD_ARG and call(ldi=d - 1) == BAD_ARG
    assert call(ws_bytes=need - 1) == _lib.MI_ERR_WORKSPACE
    assert call(n_items=2 ** 31 - 1) == _lib.MI_ERR_TOO_LARGE and call(n_q=65_535 * 64 + 1) == _lib.MI_ERR_TOO_LARGE


def _of(path):
    return [c for c in C.CASES if c.path == path]


def _has(cases, **want):
    return any(all((getattr(c, f) in v) if isinstance(v, (set, tuple)) else getattr(c, f) == v for f, v in want.items())
               for c in cases)


def test_the_table_covers_what_it_was_written_to_cover():
    f, m = _of(C.F), _of(C.M)
    assert len(f) >= 4 and len(m) >= 4
    for n in (1, 63, 64, 65, 4_097, 32_768 + 63, 40_002):       # one tile, several tiles, a partial last tile
        assert _has(f, n_items=n), n
    for n_q in (1, 63, 65, 257):
        assert _has(f, n_q=n_q), n_q
    for d in (4, 12, 64, 100, 128):
        assert _has(f, d=d), d
    for layout in ("contig", "ld+4", "halves", "same"):
        assert _has(f, layout=layout), layout
    for d in (1, 33, 132, 200):
        assert _has(m, d=d), d
    for layout in ("ld+1", "ld+1_items", "off_items", "off_users"):
        assert _has(m, d=64, layout=layout), layout
    for e in C.T.EXCLS:
        assert _has(C.CASES, excl=e), e
    for path in (f, m):
        for e in ("none", "dup", "all", "leave_k-1", "best"):
            assert _has(path, excl=e), e
        assert _has(path, values="mixed") and _has(path, values="spread")
        assert _has(path, uid="perm") and _has(path, uid="repeat")
    assert all(c.n_items >= C.T.BEST + 1 for c in C.CASES if c.excl == "best")
    assert _has(f, n_q=257, excl="all", n_items=40_002)          # the large case of the state-that-outlives-a-call test


def test_targets_mix_every_kind():
    """The drawn targets of a mixed case hold every kind, and the kinds mean what they say under the reference."""
    c = C.BY_NAME["f_65_items_d100_halves_mixed"]
    b = C.build(c, "cpu")
    scores = R.scores_fma(b["ue_ref"][b["uid"]], b["ie_ref"])
    tgt, kinds = C.targets(c, scores, b["excl"])
    assert set(kinds) == set(C.KINDS)
    rank, score, n_ex = FR.ranks(scores.numpy(), tgt.numpy(), [e.numpy() for e in b["excl"]])
    for q, kind in enumerate(kinds):
        left = c.n_items - int(n_ex[q])
        if kind == "best":
            assert rank[q] == 0
        elif kind == "worst":
            assert rank[q] == left - 1
        elif kind in ("excluded", "minus_one", "n_items"):
            assert rank[q] == -1 and (kind == "excluded" or score[q] == 0.0)
        else:
            assert 0 <= rank[q] < left


# ---- (2) the metrics ---------------------------------------------------------------------------------------------------------
def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-12)


def _compare(got, want):
    assert set(got) == set(want)
    for key, w in want.items():
        g = got[key]
        if isinstance(w, list):
            assert g.dtype == t.int64 and g.tolist() == w, key            # hits@K, filtered_rank: integers, equal
        elif isinstance(w, int):
            assert isinstance(g, int) and g == w, key
        else:
            assert isinstance(g, float) and _close(g, w), (key, g, w)


def _random_ranks(seed, n_users=40, n_items=500):
    rng = np.random.default_rng(seed)
    pos_of, rank, n_ex, gt_len = [], [], [], []
    for u in range(n_users):
        m = int(rng.integers(1, 7))
        r = rng.choice(n_items - 60, size=m, replace=False)              # a user's pairs are distinct items: distinct ranks
        if u < 6:
            r = rng.choice(12, size=m, replace=False)                     # some users crowd the top places
        gone = rng.random(len(r)) < 0.2
        if u == 3:
            gone[:] = True                                                # a user whose pairs are all -1
        if u == 4:
            gone[:] = False
        r = np.where(gone, -1, r)
        e = int(rng.integers(0, 50))
        pos_of += [u] * len(r)
        rank += r.tolist()
        n_ex += [e] * len(r)
        gt_len.append(len(r) + int(rng.integers(0, 3)))                   # repeated edges count in |GT|
    order = rng.permutation(len(rank))                                    # the pairs need not be grouped by user
    pick = lambda x: [x[i] for i in order]
    return pick(pos_of), pick(rank), n_items, pick(n_ex), gt_len


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_full_rank_metrics_equal_the_loop_reference(seed, filtered):
    from laplace_amd.utils.metrics_lightgcn import full_rank_metrics
    pos_of, rank, n_items, n_ex, gt_len = _random_ranks(seed)
    assert -1 in rank
    ks = (1, 12, 256, n_items)
    got = full_rank_metrics(t.tensor(pos_of), t.tensor(rank, dtype=t.int32), n_items, t.tensor(n_ex, dtype=t.int32),
                            t.tensor(gt_len), ks=ks, filtered=filtered)
    _compare(got, FR.metrics(pos_of, rank, n_items, n_ex, gt_len, ks, filtered=filtered))
    assert got["excluded_pairs"] == sum(1 for r in rank if r < 0) > 0


def test_no_pair_left_is_nan_not_an_error():
    from laplace_amd.utils.metrics_lightgcn import full_rank_metrics
    got = full_rank_metrics(t.tensor([0, 1]), t.tensor([-1, -1], dtype=t.int32), 10, t.tensor([1, 1], dtype=t.int32),
                            t.tensor([1, 1]), ks=(3,))
    _compare(got, FR.metrics([0, 1], [-1, -1], 10, [1, 1], [1, 1], (3,)))
    assert got["excluded_pairs"] == 2 and got["recall@3"] == 0.0 and math.isnan(got["mrr"]) and math.isnan(got["auc"])
    with pytest.raises(ValueError):
        full_rank_metrics(t.tensor([0]), t.tensor([0], dtype=t.int32), 10, t.tensor([0], dtype=t.int32), t.tensor([1]), ks=(11,))


def test_hand_computed_example():
    """Three users, seven pairs, ten items.  user 0: ranks 0, 2, 5, one item excluded; user 1: rank 1 and a pair that is
    itself excluded (-1), two items excluded; user 2: ranks 3 and 7, nothing excluded."""
    from laplace_amd.utils.metrics_lightgcn import full_rank_metrics
    pos_of = t.tensor([0, 0, 0, 1, 1, 2, 2])
    rank = t.tensor([5, 0, 2, 1, -1, 7, 3], dtype=t.int32)
    n_ex = t.tensor([1, 1, 1, 2, 2, 0, 0], dtype=t.int32)
    gt_len = t.tensor([3, 2, 2])
    m = full_rank_metrics(pos_of, rank, 10, n_ex, gt_len, ks=(3,))
    Fr = Fraction
    assert m["excluded_pairs"] == 1 and m["pairs"] == 6
    assert m["hits@3"].tolist() == [2, 1, 0]
    assert m["filtered_rank"].tolist() == [3, 0, 1, 1, -1, 6, 3]
    # map@3: user 0 (1/1 + 2/3) / min(3, 3); user 1 (1/2) / min(3, 1); user 2 nothing inside 3
    assert _close(m["map@3"], float((Fr(5, 3) / 3 + Fr(1, 2) + 0) / 3)) and _close(m["map@3"], 19 / 54)
    assert _close(m["mrr"], float((Fr(1) + Fr(1, 2) + Fr(1, 4)) / 3))
    assert _close(m["mean_rank"], 3.0)
    # auc: user 0 over 10 - 1 - 3 = 6 other items, user 1 over 10 - 2 - 1 = 7, user 2 over 10 - 0 - 2 = 8
    auc = (Fr(6, 6) + Fr(5, 6) + Fr(3, 6) + Fr(6, 7) + Fr(5, 8) + Fr(2, 8)) / 6
    assert _close(m["auc"], float(auc))
    assert _close(m["recall@3"], float((Fr(2, 3) + Fr(1, 2)) / 3)) and _close(m["precision@3"], float(Fr(3, 3) / 3))
    f = full_rank_metrics(pos_of, rank, 10, n_ex, gt_len, ks=(3,), filtered=True)
    assert f["hits@3"].tolist() == [2, 1, 0] and f["filtered_rank"].tolist() == m["filtered_rank"].tolist()
    assert _close(f["mean_rank"], (3 + 0 + 1 + 1 + 6 + 3) / 6) and _close(f["auc"], m["auc"])
    assert _close(f["map@3"], float(((Fr(1, 1) + Fr(2, 2)) / 3 + Fr(1, 2) + 0) / 3))


@pytest.fixture(scope="module")
def small_split():
    """60 users x 600 items, d = 8: oracle scores, exclusions, held-out edges with repeats, the reference's ranks."""
    g = t.Generator().manual_seed(11)
    U, I, d = 60, 600, 8
    ue, ie = t.randn(U, d, generator=g), t.randn(I, d, generator=g)
    ie[::7] = ie[3]                                                       # score ties across items
    scores = R.scores_fma(ue, ie)
    excl = [t.randperm(I, generator=g)[: int(t.randint(0, 40, (1,), generator=g))] for _ in range(U)]
    edges = []
    for u in range(U):
        m = int(t.randint(1, 6, (1,), generator=g))
        best = scores[u].topk(300).indices
        items = best[t.randperm(300, generator=g)[:m]].tolist()
        if u % 5 == 0 and len(excl[u]):
            items[0] = int(excl[u][0])                                    # a held-out pair that is itself excluded
        if u % 4 == 0:
            items.append(items[-1])                                       # a repeated edge: counted twice in |GT|
        edges += [(u, i) for i in items]
    pairs = sorted(set(edges))
    pos_of = np.array([u for u, _ in pairs])
    items = np.array([i for _, i in pairs])
    rank, _, n_ex = FR.ranks(scores.numpy()[pos_of], items, [excl[u].numpy() for u in pos_of])
    gt_len = np.bincount([u for u, _ in edges], minlength=U)
    return dict(scores=scores, excl=excl, pairs=pairs, pos_of=pos_of, items=items, rank=rank, n_ex=n_ex, gt_len=gt_len, n_items=I)


@pytest.mark.parametrize("k", [1, 12, 256])
def test_at_k_metrics_from_ranks_equal_rank_metrics_on_the_top_k_hit_matrix(small_split, k):
    from laplace_amd.utils.metrics_lightgcn import full_rank_metrics, rank_metrics
    s = small_split
    top = R.topk_excl_exact(s["scores"], s["excl"], k)
    truth = set(s["pairs"])
    r = t.tensor([[(u, int(i)) in truth for i in row] for u, row in enumerate(top.tolist())])
    want = rank_metrics(r, t.from_numpy(s["gt_len"]), k)
    got = full_rank_metrics(t.from_numpy(s["pos_of"]), t.from_numpy(s["rank"]), s["n_items"], t.from_numpy(s["n_ex"]),
                            t.from_numpy(s["gt_len"]), ks=(k,))
    assert got["excluded_pairs"] > 0
    assert got[f"hits@{k}"].tolist() == r.sum(1).tolist()
    for name, w in zip(("recall", "precision", "ndcg"), want):
        assert abs(got[f"{name}@{k}"] - w) <= 1e-6, (name, got[f"{name}@{k}"], w)   # rank_metrics works in float32
    # and the position: the pair stands in column c of the list iff rank == c < k
    for p, (u, i) in enumerate(s["pairs"]):
        row = top[u].tolist()
        assert (row.index(i) if i in row else -1) == (int(s["rank"][p]) if 0 <= s["rank"][p] < k else -1)
