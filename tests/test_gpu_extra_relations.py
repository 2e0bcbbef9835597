"""GPU: attribute node types in the device sampler's batches (Config.other_edge_types; mi_sampler_count_relations_async,
mi_sampler_emit_relations) against the NumPy mirror of the rule (tests/extra_relations_emulation.py), tensor for tensor.

The graph is the smallest that can still go wrong: 40 users, 30 articles, about 150 edges, batch_size 3, two hops, fan-out
4, two relations at once.  Relation A has 5 targets, one per article; relation B has 70 (three bitmap words, ids 31 | 32 and
63 | 64 on both sides of the word borders), rows of 0, 1 and 3 targets, and articles without any."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t

import extra_relations_emulation as RE

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIPARTITE = ("user_ids", "article_ids", "edge_index", "edge_label_index", "edge_label", "user_ptr", "article_ptr")


def _sampler(relations=True, train=True, prefetch=True, empty_b=False, seed=77):
    from laplace_amd.data.device_sampler import DeviceGraphSampler
    g, users, articles, cfg, rels = RE.make_graph(("A", "B"), empty_b=empty_b)
    if not relations:
        cfg = SimpleNamespace(**{**vars(cfg), "other_edge_types": []})
    smp = DeviceGraphSampler(cfg, g, users, articles, device=DEV, seed=seed, prefetch=prefetch, train=train,
                             matchers=None if train else [RE.IslandMatcher()])
    return smp, g, ({} if empty_b else rels)


def _csrs(rows_by_key):
    return {key: RE.rel_csr(rows, RE.A) for key, rows in rows_by_key.items()}


def _check_against_emulation(article_ids, article_ptr, got, rel_ptr, rel_idx, what):
    """got: T_ids, T_ptr, edge3 [3, ne], (by article, by target) CSRs.  Returns the emulation's result."""
    want = RE.emulate(article_ids.cpu().numpy(), article_ptr.cpu().numpy(), rel_ptr, rel_idx)
    t_ids, t_ptr, e3, (by_a, by_t) = got
    eq = lambda x, y: x.dtype == y.dtype and x.shape == y.shape and t.equal(x.cpu(), y)
    assert eq(t_ids, t.from_numpy(want["T_ids"])), what
    assert eq(t_ptr, t.from_numpy(want["T_ptr"])), what
    assert e3.shape[0] == 3 and eq(e3[0:2], t.from_numpy(want["edge_index"])) and t.equal(e3[2], e3[0]), what
    for csr, key, n_rows, n_cols in ((by_a, "by_article", article_ids.numel(), t_ids.numel()),
                                     (by_t, "by_target", t_ids.numel(), article_ids.numel())):
        assert (csr.n_rows, csr.n_cols) == (n_rows, n_cols), what
        assert eq(csr.rowptr, t.from_numpy(want[key][0])) and eq(csr.col, t.from_numpy(want[key][1])), (what, key)
    return want


def _seeds(step):
    return t.tensor([(step * 7) % 37, (step * 11 + 3) % 37, 37 + step % 3])       # the last one is an island user


@pytest.mark.parametrize("train", [True, False])
def test_emitted_relations_equal_the_emulation_and_the_walk_is_unchanged(train):
    smp, _, rels = _sampler(train=train)
    plain, _, _ = _sampler(relations=False, train=train)
    csrs = _csrs(rels)
    no_target, shared = 0, 0
    for step in range(5):
        raw = smp.sample(_seeds(step), step=step, raw=True)
        ref = plain.sample(_seeds(step), step=step, raw=True)
        for k in BIPARTITE:
            assert raw[k].shape == ref[k].shape and t.equal(raw[k], ref[k]), (step, k)
        for k in ("csr_by_customer", "csr_by_article"):
            assert t.equal(raw[k].rowptr, ref[k].rowptr) and t.equal(raw[k].col, ref[k].col), (step, k)
        assert "relations" not in ref and list(raw["relations"]) == [RE.REL_A, RE.REL_B]
        for key, r in raw["relations"].items():
            assert r["edge_index"].data_ptr() == r["edge3"].data_ptr()
            want = _check_against_emulation(raw["article_ids"], raw["article_ptr"],
                                            (r["T_ids"], r["T_ptr"], r["edge3"], (r["csr_by_article"], r["csr_by_target"])),
                                            *csrs[key], (step, key))
            if key == RE.REL_A:   # exactly one target per article
                assert want["edge_index"].shape[1] == raw["article_ids"].numel()
            else:
                per = np.diff(want["T_ptr"])
                no_target += int((per == 0).sum())
                sets = [set(want["T_ids"][want["T_ptr"][s]:want["T_ptr"][s + 1]].tolist()) for s in range(3)]
                shared += len((sets[0] & sets[1]) | (sets[0] & sets[2]) | (sets[1] & sets[2]))
    assert shared > 0                      # a target reached from the articles of two samples: one node in each
    if not train:                          # the island user's candidates and purchases have no relation-B target
        assert no_target >= 5


def _fields(batch, keys):
    """Every tensor of a batch: the bipartite part as tests/test_gpu_abandoned_iterators.py lists it, then the relations."""
    from laplace_amd.utils.constants import Constants
    out = []
    for nt in (Constants.node_user, Constants.node_item):
        out += [batch[nt].x, batch[nt].n_id]
    for k in ("edge_index", "edge_label_index", "edge_label"):
        out += [batch[Constants.edge_key][k], batch[Constants.rev_edge_key][k]]
    for csr in batch[Constants.edge_key].edge_index._sorted_csr:
        out += [csr.rowptr, csr.col]
    out += [batch._user_ptr, batch._article_ptr]
    for key in keys:
        T, rev = key[2], (key[2], "rev_" + key[1], key[0])
        fwd = batch[key].edge_index
        assert list(batch[key]) == ["edge_index"] and list(batch[rev]) == ["edge_index"]    # no edge_label*
        assert batch[rev].edge_index._reverse_of is fwd
        out += [batch[T].x, batch[T].n_id, batch[T].ptr, fwd, batch[rev].edge_index]
        for csr in fwd._sorted_csr:
            out += [csr.rowptr, csr.col]
    return out


def _same(a, b, keys, what):
    assert a.node_types == b.node_types and a.edge_types == b.edge_types
    fa, fb = _fields(a, keys), _fields(b, keys)
    assert len(fa) == len(fb)
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and t.equal(x, y), (what, i)


def _batch_matches_emulation(batch, g, csrs, what):
    for key, (ptr, idx) in csrs.items():
        T, rev = key[2], (key[2], "rev_" + key[1], key[0])
        fwd = batch[key].edge_index
        assert t.equal(batch[rev].edge_index, fwd.flip(0)), what
        assert t.equal(batch[T].x.cpu(), g[T].x[batch[T].n_id.cpu()]), what
        e3 = t.cat([fwd, fwd[0:1]])
        _check_against_emulation(batch[RE.ARTICLE].n_id, batch._article_ptr, (batch[T].n_id, batch[T].ptr, e3, fwd._sorted_csr),
                                 ptr, idx, (what, key))


def test_every_path_hands_out_the_same_batches():
    serial, g, rels = _sampler(prefetch=False)
    keys = list(rels)
    csrs = _csrs(rels)
    n_batches = (RE.U + 2) // 3
    want = list(serial)                                  # the serial epoch: steps 0..13, the last batch one user short
    assert len(want) == n_batches and want[-1]._seed_users.numel() == 1
    assert want[0].node_types == [RE.CUSTOMER, RE.ARTICLE, RE.REL_A[2], RE.REL_B[2]]
    for i, b in enumerate(want):
        _batch_matches_emulation(b, g, csrs, ("serial", i))
    for mode in (True, "thread"):
        ahead, _, _ = _sampler(prefetch=mode)
        got = list(ahead)
        assert len(got) == n_batches and ahead.step == n_batches
        for i, (a, b) in enumerate(zip(want, got)):
            _same(a, b, keys, (mode, i))
        users = t.tensor([5, 38, 0, 17, 39, 2, 30])      # 3 + 3 + 1
        mine = list(ahead.iter_users(users))
        assert [b._seed_users.numel() for b in mine] == [3, 3, 1]
        for i, b in enumerate(mine):
            _same(serial.sample(users[3 * i:3 * i + 3], step=n_batches + i), b, keys, (mode, "iter_users", i))


@pytest.mark.parametrize("mode", [True, "thread"])
def test_no_bit_of_a_batch_reaches_the_next(mode):
    """The per-sample target bitmaps live in a ring of workspaces that the next batches reuse: two epochs in a row, and an
    iterator left after one batch (its successors were counted and never emitted) and started again."""
    ahead, g, rels = _sampler(prefetch=mode)
    csrs = _csrs(rels)
    n = 0
    for epoch in range(2):
        for b in ahead:
            _batch_matches_emulation(b, g, csrs, ("epoch", epoch, n))
            n += 1
    it = iter(ahead)
    first = next(it)
    it.close()
    del it
    gc.collect()
    _batch_matches_emulation(first, g, csrs, "before the break")
    assert ahead.step == n + 1
    for i, b in enumerate(ahead):
        _batch_matches_emulation(b, g, csrs, ("after the break", i))


def _encoder_inputs(batch, tables):
    x = {nt: tables[nt][batch[nt].n_id] for nt in batch.node_types}
    return x, batch.edge_index_dict


@pytest.mark.parametrize("conv_aggr", ["add", "mean", "max"])
def test_a_relation_without_any_edge(conv_aggr):
    from laplace_amd.model.encoder_decoder import HeteroGNNEncoder
    from laplace_amd.model.layers import get_SAGEConv_layers
    smp, g, _ = _sampler(empty_b=True)
    batch = smp.sample(_seeds(0), step=0)
    T = RE.REL_B[2]
    assert batch[T].x.shape == (0, 2) and batch[T].n_id.shape == (0,) and batch[T].ptr.tolist() == [0, 0, 0, 0]
    for key in (RE.REL_B, (T, "rev_has_tag", RE.ARTICLE)):
        assert batch[key].edge_index.shape == (2, 0) and batch[key].edge_index.dtype == t.int64
    by_a, by_t = batch[RE.REL_B].edge_index._sorted_csr
    n_a = batch[RE.ARTICLE].x.shape[0]
    assert by_a.rowptr.tolist() == [0] * (n_a + 1) and by_t.rowptr.tolist() == [0] and by_a.nnz == by_t.nnz == 0
    assert batch[RE.REL_A].edge_index.shape == (2, n_a)          # the other relation is not disturbed
    gen = t.Generator().manual_seed(2)
    sizes = {RE.CUSTOMER: RE.U, RE.ARTICLE: RE.A, RE.REL_A[2]: RE.N_TA, T: RE.N_TB}
    tables = {nt: t.randn(n, 12, generator=gen).to(DEV).requires_grad_(True) for nt, n in sizes.items()}
    t.manual_seed(1)
    enc = HeteroGNNEncoder(get_SAGEConv_layers(2, 16, 8, conv_aggr), batch.metadata(), "sum", 0.0, None).to(DEV)
    out = enc(*_encoder_inputs(batch, tables))
    assert set(out) == set(sizes) and out[T].shape == (0, 8) and out[RE.ARTICLE].shape == (n_a, 8)
    sum(v.sum() for v in out.values()).backward()
    assert all(bool(t.isfinite(v).all()) for v in out.values())
    assert all(p.grad is not None and bool(t.isfinite(p.grad).all()) for p in enc.parameters())
    assert float(tables[T].grad.abs().max()) == 0.0 and float(tables[RE.ARTICLE].grad.abs().max()) > 0.0


@pytest.mark.parametrize("hetero_aggr", ["sum", "max"])
def test_encoder_on_sampled_batches_against_the_oracle(hetero_aggr):
    """The comparison of test_to_hetero_three_relations_per_destination (tests/test_gpu_ranker.py), with its tolerances, on a
    batch the sampler made: three relations arrive at `article`, so heterogeneous_prop_agg_type is at work."""
    from oracle import ranker_ref as RR
    from laplace_amd.model.encoder_decoder import HeteroGNNEncoder
    from laplace_amd.model.layers import get_SAGEConv_layers
    smp, g, rels = _sampler()
    batch = smp.sample(_seeds(1), step=1)
    first = batch
    assert len(first.metadata()[1]) == 6
    gen = t.Generator().manual_seed(11)
    sizes = {RE.CUSTOMER: RE.U, RE.ARTICLE: RE.A, RE.REL_A[2]: RE.N_TA, RE.REL_B[2]: RE.N_TB}
    cpu_tables = {nt: t.randn(n, 24, generator=gen) for nt, n in sizes.items()}
    tables = {nt: v.clone().to(DEV).requires_grad_(True) for nt, v in cpu_tables.items()}
    ref_tables = {nt: v.clone().requires_grad_(True) for nt, v in cpu_tables.items()}
    t.manual_seed(3)
    enc = HeteroGNNEncoder(get_SAGEConv_layers(2, 32, 16, "add"), first.metadata(), hetero_aggr, 0.0, None).to(DEV)
    x, ei = _encoder_inputs(batch, tables)
    out = enc(x, ei)
    dims = [{k: (c.lin_l.in_features, c.lin_r.in_features, c.out_channels) for k, c in convs.items()} for convs in enc.layers]
    ref = RR.HeteroEncoderRef(dims, "add", hetero_aggr, None)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in enc.state_dict().items()})
    want = ref({nt: ref_tables[nt][batch[nt].n_id.cpu()] for nt in batch.node_types}, {k: v.cpu() for k, v in ei.items()})
    assert set(out) == set(want) == set(sizes)
    for k in want:
        scale = float(want[k].abs().max()) + 1e-6
        assert (out[k].detach().cpu() - want[k].detach()).abs().max() <= 1e-5 * max(1.0, scale), (k, hetero_aggr)
    w = {k: t.randn(v.shape, generator=gen) for k, v in want.items()}
    sum((out[k] * w[k].to(DEV)).sum() for k in out).backward()
    sum((want[k] * w[k]).sum() for k in want).backward()
    for (n, p), (_, pr) in zip(enc.named_parameters(), ref.named_parameters()):
        scale = float(pr.grad.abs().max()) + 1e-6
        assert float((p.grad.cpu() - pr.grad).abs().max()) <= 2e-4 * scale + 1e-6, (n, hetero_aggr)
    for T in (RE.REL_A[2], RE.REL_B[2]):            # information reaches the articles through the new relations, and back
        assert float(tables[T].grad.abs().max()) > 0.0
        scale = float(ref_tables[T].grad.abs().max()) + 1e-6
        assert float((tables[T].grad.cpu() - ref_tables[T].grad).abs().max()) <= 2e-4 * scale + 1e-6, T
    # the emitted CSRs are the ones the encoder would build from edge_index: without them the output has the same bits
    stripped = {}
    for k, v in ei.items():
        stripped[k] = v.clone()
        if getattr(v, "_reverse_of", None) is not None:
            stripped[k]._reverse_of = stripped[(k[2], k[1][4:], k[0])]
    assert all(not hasattr(v, "_sorted_csr") for v in stripped.values())
    again = enc({k: v.detach() for k, v in x.items()}, stripped)
    for k in out:
        assert t.equal(again[k], out[k]), k


def _config(cfg):
    from laplace_amd.config import Config
    return Config(wandb_enabled=False, epochs=2, hidden_layer_size=16, encoder_layer_output_size=8, k=cfg.k, num_gnn_layers=2,
                  num_linear_layers=2, learning_rate=0.01, conv_agg_type="add", heterogeneous_prop_agg_type="sum", save_model=False,
                  eval_every=1, save_every=1.0, batch_size=cfg.batch_size, num_neighbors=cfg.num_neighbors,
                  n_hop_neighbors=cfg.n_hop_neighbors, num_workers=1, candidate_pool_size=20, positive_edges_ratio=0.5,
                  negative_edges_ratio=3.0, batch_norm=True, matchers="fashion", p_dropout_edges=0.0, p_dropout_features=0.1,
                  default_edge_types=[(RE.CUSTOMER, "buys", RE.ARTICLE)], other_edge_types=cfg.other_edge_types,
                  node_types=cfg.node_types)


def test_pipeline_end_to_end_and_what_declines():
    from laplace_amd.model.encoder_decoder import Encoder_Decoder_Model
    from laplace_amd.model.layers import get_SAGEConv_layers, get_linear_layers
    from laplace_amd.ranker_native import NativeRankerForward, NativeRankerStep
    from laplace_amd.run_pipeline import run_pipeline
    from laplace_amd.training import train_with_dataloader
    from laplace_amd.utils.get_info import get_feature_info
    g, users, articles, cfg, _ = RE.make_graph(("A", "B"))
    config = _config(cfg)
    stats = run_pipeline(config, splits={k: (g, users, articles) for k in ("train", "val", "test")}, device=DEV, verbose=False)
    assert np.isfinite(stats.loss)
    # the same model on the device sampler's batches: the native executors decline, the autograd path trains
    smp, _, _ = _sampler()
    first = smp.sample(_seeds(0), step=0)
    t.manual_seed(0)
    model = Encoder_Decoder_Model(get_SAGEConv_layers(2, 16, 8, "add"), get_linear_layers(2, 16, 16, 1), get_feature_info(g),
                                  first.metadata(), True, "sum", True, 0.0, 0.1).to(DEV)
    model.initialize_encoder_input_size(first)
    opt = t.optim.Adam(model.parameters(), lr=0.01)
    assert NativeRankerStep.unsupported_reason(model, opt) == "node types other than [customer, article]"
    assert not NativeRankerStep.supports(model, opt) and not NativeRankerForward.supports(model)
    model.train()
    losses = train_with_dataloader(model, opt, smp, 0, DEV)
    assert len(losses) == len(smp) and np.isfinite(losses).all()
    assert any("colour_group_code" in n for n, _ in model.named_parameters())
