"""GPU: ops.rank_of_items (csrc/rank.hip, K10r of include/laplace_hip.h) on the case table of tests/rank_cases.py, and the
metrics built on it.  Ranks, distinct-exclusion counts and the bits of the target scores equal tests/full_rank_reference.py on
the oracle's fma-chain scores — nothing about the kernel has a tolerance.  The dispatcher's own decision function says which
kernel ran.  Then: agreement with top-K (rank == column), chunked calls, repeated calls, state that outlives a call in a shared
workspace, get_full_rank_metrics_lightgcn against get_metrics_lightgcn's top-K lists, and the pipeline's JSON."""
import functools
import json
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch as t

from oracle import lightgcn_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_rank_reference as FR  # noqa: E402
import rank_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """The case's tensors, targets and reference, made once and shared by the tests below (none of them writes to it)."""
    from laplace_amd import ops
    c = C.BY_NAME[name]
    b = C.build(c, DEV)
    scores = R.scores_fma(b["ue_ref"][b["uid"]], b["ie_ref"])
    if b["need_scores"]:
        C.finish_excl(c, b, scores)
    target, kinds = C.targets(c, scores, b["excl"])
    excl_np = [e.numpy() for e in b["excl"]] if b["excl"] is not None else None
    rank, score, n_ex = FR.ranks(scores.numpy(), target.numpy(), excl_np)
    ex = None if b["rowptr"] is None else ops.DeviceCSR(c.n_q, c.n_items, b["rowptr"].to(DEV), b["col"].to(DEV))
    return dict(b=b, scores=scores, target=target, kinds=kinds, ex=ex, uid=b["uid"].to(DEV), tgt=target.to(DEV),
                rank=t.from_numpy(rank), score=t.from_numpy(score), n_ex=t.from_numpy(n_ex))


def _call(p, **kw):
    from laplace_amd import ops
    return ops.rank_of_items(p["uid"], p["tgt"], p["b"]["ue"], p["b"]["ie"], p["ex"], want_scores=True, want_n_excluded=True, **kw)


def _assert_equals_reference(p, got, what=""):
    rank, score, n_ex = (x.cpu() for x in got)
    assert rank.dtype == t.int32 and n_ex.dtype == t.int32 and score.dtype == t.float32
    bad = (rank != p["rank"]).nonzero().view(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {rank.numel()} ranks differ, first: row {int(bad[0])} "
                              f"({p['kinds'][int(bad[0])]}) got {int(rank[bad[0]])} want {int(p['rank'][bad[0]])}")
    assert t.equal(n_ex, p["n_ex"]), what
    assert t.equal(score.view(t.int32), p["score"].view(t.int32)), what          # the bits


# ---- 1: every case; 4: two calls return equal tensors ------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_case_runs_its_declared_path_and_equals_the_reference(case):
    from laplace_amd import ops
    c = case
    p = _prepared(c.name)
    ue, ie = p["b"]["ue"], p["b"]["ie"]
    up, ldu, ip, ldi = C.layout_of(c, 0, 0)
    assert ue.data_ptr() % 16 == up % 16 and ie.data_ptr() % 16 == ip % 16
    assert ops._rows_ok(ue, "ue") == ldu and ops._rows_ok(ie, "ie") == ldi
    got_path = ops.rank_path(ue, ie)
    assert got_path == c.path, (C.PATH_NAMES.get(got_path, got_path), C.PATH_NAMES[c.path])
    # the targets hold what the table promises: in and out of range, excluded where a row excludes anything
    kinds = set(p["kinds"])
    assert {"minus_one", "n_items"} <= kinds or c.n_q < 7
    if c.excl == "all":
        assert int(p["rank"][0]) == -1 and int(p["n_ex"][0]) == c.n_items
    got = _call(p)
    _assert_equals_reference(p, got, "first call")
    again = _call(p)
    for a, b in zip(got, again):
        assert t.equal(a, b)
    # the optional outputs are optional, and the tables were not written to
    only = ops.rank_of_items(p["uid"], p["tgt"], ue, ie, p["ex"])
    assert isinstance(only, t.Tensor) and t.equal(only, got[0])
    assert t.equal(ue.cpu(), p["b"]["ue_ref"]) and t.equal(ie.cpu(), p["b"]["ie_ref"])


# ---- 2: agreement with top-K -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f_partial_last_tile_d64_best", "f_4097_items_d128_mixed_leave_k-1", "m_d33_mixed_dup",
                                  "f_63_items_d12_pinsage_form"])
def test_rank_is_the_column_of_the_top_k_list(name):
    """One row per non-pad entry of topk_excl's list, with the same user and the same exclusion row: rank == column.  In the
    mixed cases whole rows tie and only the item id decides."""
    from laplace_amd import ops
    c = C.BY_NAME[name]
    p = _prepared(name)
    ue, ie = p["b"]["ue"], p["b"]["ie"]
    k = min(c.k, c.n_items)
    top = ops.topk_excl(p["uid"], ue, ie, k, p["ex"]).cpu()
    q_of, col_of = (top >= 0).nonzero(as_tuple=True)
    assert q_of.numel() > 0
    if c.excl == "leave_k-1":
        assert int((top[0] >= 0).sum()) == k - 1
    ex = None
    if p["b"]["excl"] is not None:
        lists = [p["b"]["excl"][int(q)] for q in q_of]
        lens = t.tensor([len(e) for e in lists], dtype=t.int64)
        rowptr = t.cat([t.zeros(1, dtype=t.int64), lens.cumsum(0)]).to(t.int32)
        ex = ops.DeviceCSR(q_of.numel(), c.n_items, rowptr.to(DEV), t.cat(lists).to(t.int32).to(DEV))
    rank = ops.rank_of_items(p["uid"][q_of.to(DEV)].contiguous(), top[q_of, col_of].to(DEV), ue, ie, ex).cpu()
    assert t.equal(rank.to(t.int64), col_of)


# ---- 3: chunking -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f_4097_items_d128_mixed_leave_k-1", "m_d132_all"])
def test_chunked_call_gives_the_same_tensors(name):
    p = _prepared(name)
    assert C.BY_NAME[name].n_q == 257
    whole = _call(p)
    for chunk in (100, 64, 1000):                       # three launches with a short last one; whole panels; one launch
        cut = _call(p, chunk=chunk)
        for a, b in zip(whole, cut):
            assert t.equal(a, b), chunk
    _assert_equals_reference(p, whole, "whole")


# ---- 5: state that outlives a call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large,small", [("f_40002_items_d128_spread_all", "f_64_items_d128_mixed_none"),
                                         ("m_d132_all", "m_d64_ld_plus_1_none")])
def test_shared_workspace_carries_nothing_from_call_to_call(large, small):
    """A large case whose row 0 sets every bit of its bitmap row, then a small case without exclusions, then the first again,
    all in ONE workspace: a bitmap, a counter or a target that is not reset per call shows as a wrong rank."""
    from laplace_amd import _lib
    L = _lib.lib()
    cl, cs = C.BY_NAME[large], C.BY_NAME[small]
    assert cl.excl == "all" and cs.excl == "none"
    need = max(int(L.mi_rank_items_workspace_bytes(c.n_q, c.n_items)) for c in (cl, cs))
    ws = t.empty(need, dtype=t.uint8, device=DEV)
    ws.fill_(0xFF)                                       # a workspace that starts dirty
    for name in (large, small, large):
        p = _prepared(name)
        _assert_equals_reference(p, _call(p, ws=ws), name)
    with pytest.raises(_lib.MiError):
        _call(_prepared(large), ws=ws[:1024])


# ---- 6: the metrics on a planted graph ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """300 users x 500 items in 8 taste groups, d = 32, ten training steps; the last fifth of the edges is held out, and some
    held-out edges are listed twice (|GT| counts them twice, the pairs are distinct)."""
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    from test_gpu_acceptance import _tastes_graph
    U, I = 300, 500
    pairs = t.from_numpy(_tastes_graph(U, I, 3000, seed=7).T.copy())
    train_e, test_e = pairs[:, :2400].to(DEV), pairs[:, 2400:]
    test_e = t.cat([test_e, test_e[:, :40]], dim=1).to(DEV)
    t.manual_seed(0)
    model = LightGCN(U, I, 32, 2).to(DEV)
    inter = Interactions(train_e, U, I)
    adj = inter.adjacency("bipartite")
    tr = LightGCNTrainer(model, adj, inter, lr=1e-2, Lambda=1e-6, batch_size=256, seed=3, objective="bpr")
    for _ in range(10):
        tr.step()
    tr.finish()
    model.eval()
    with t.no_grad():
        uf, _, itf, _ = model.forward(adj)
    return dict(model=model, train=train_e, test=test_e, propagated=(uf.contiguous(), itf.contiguous()), n_items=I)


@pytest.mark.parametrize("tables", ["layer0", "propagated"])
def test_full_rank_metrics_agree_with_the_top_k_metrics(planted, tables):
    from laplace_amd.utils.metrics_lightgcn import (get_full_rank_metrics_lightgcn, get_metrics_lightgcn, ranks_for_edges,
                                                    topk_for_users)
    g = planted
    emb = g["propagated"] if tables == "propagated" else None
    ks = (12, 256)
    full = get_full_rank_metrics_lightgcn(g["model"], g["test"], [g["train"]], ks, embeddings=emb)
    ue, ie = emb if emb is not None else (g["model"].users_emb.weight.detach(), g["model"].items_emb.weight.detach())
    users = g["test"][0].unique()
    pos_of = t.searchsorted(users, g["test"][0])
    truth = t.unique(pos_of * g["n_items"] + g["test"][1])
    assert truth.numel() < g["test"].shape[1]                                    # the repeated edges are there
    assert full["pairs"] + full["excluded_pairs"] == truth.numel()
    for k in ks:
        top = topk_for_users(ue, ie, users, g["train"], k)
        r = t.isin(t.arange(users.numel(), device=DEV)[:, None] * g["n_items"] + top, truth) & (top >= 0)
        assert t.equal(full[f"hits@{k}"], r.sum(1))                              # per user, exactly
        want = get_metrics_lightgcn(g["model"], g["test"], [g["train"]], k, embeddings=emb)
        for name, w in zip(("recall", "precision", "ndcg"), want):
            assert abs(full[f"{name}@{k}"] - w) <= 1e-6, (tables, name, k, full[f"{name}@{k}"], w)
    assert 0.0 < full["mrr"] <= 1.0 and 0.0 <= full["auc"] <= 1.0 and 0.0 <= full["mean_rank"] < g["n_items"]
    # filtered: integer post-processing of the same ranks
    filt = get_full_rank_metrics_lightgcn(g["model"], g["test"], [g["train"]], ks, embeddings=emb, filtered=True)
    assert t.equal(filt["filtered_rank"], full["filtered_rank"]) and filt["auc"] == full["auc"]
    assert filt["mean_rank"] <= full["mean_rank"] and bool((filt["hits@12"] >= full["hits@12"]).all())
    # and the loop reference on the ranks the device returned
    users2, pos2, items2, ranks, n_ex = ranks_for_edges(ue, ie, g["test"], g["train"])
    assert t.equal(users2, users) and t.equal(pos2 * g["n_items"] + items2, truth)
    gt_len = t.bincount(pos_of, minlength=users.numel())
    want = FR.metrics(pos2.tolist(), ranks.tolist(), g["n_items"], n_ex.tolist(), gt_len.tolist(), ks)
    for key, w in want.items():
        if isinstance(w, float):
            assert abs(full[key] - w) <= 1e-12 * max(1.0, abs(w)), key
        elif isinstance(w, list):
            assert full[key].tolist() == w, key
        else:
            assert full[key] == w, key


# ---- 7: the pipeline ---------------------------------------------------------------------------------------------------------
def test_pipeline_writes_the_full_rank_json_and_leaves_the_stats_alone(tmp_path):
    from laplace_amd.config import lightgcn_config
    from laplace_amd.run_pipeline_lightgcn import train
    from test_gpu_acceptance import _tastes_graph
    cfg = replace(lightgcn_config, epochs=20, k=12, hidden_layer_size=32, learning_rate=1e-2, save_model=False, batch_size=128,
                  num_iterations=2, eval_every=10, lr_decay_every=10, Lambda=1e-6, show_graph=False, num_recommendations=50)
    ei = t.from_numpy(_tastes_graph(300, 500, 3000, seed=7).T.copy())
    kw = dict(edge_index=ei, num_users=300, num_articles=500, compat="bipartite", device=DEV, seed=5, verbose=False,
              objective="bpr", predictor="propagated")
    d = str(tmp_path / "with")
    stats = train(cfg, save_dir=d, full_rank_ks=(12, 50), **kw)
    full = json.load(open(os.path.join(d, "full_rank_metrics.json")))
    for key in ("recall@12", "precision@12", "ndcg@12", "map@12", "recall@50", "map@50", "mrr", "mean_rank", "auc",
                "excluded_pairs", "pairs"):
        assert key in full and np.isfinite(full[key]), key
    assert abs(full["recall@12"] - stats.recall_test) <= 1e-6
    assert abs(full["precision@12"] - stats.precision_test) <= 1e-6
    assert full["recall@50"] >= full["recall@12"]
    d2 = str(tmp_path / "without")
    plain = train(cfg, save_dir=d2, **kw)
    assert plain == stats                                                       # the same Stats as before
    assert not os.path.exists(os.path.join(d2, "full_rank_metrics.json"))
