"""GPU: PinSAGE's item feature projector (mi_pinsage_project_f32 / _bwd_f32) against the torch twin of
tests/test_pinsage_features_cpu.py, the featured model's autograd and native iterations against PinSAGERef + twin on the
mirror's batches, the featured catalogue pass, and what the feature is for: items without interactions."""
import numpy as np
import pytest
import torch as t

from oracle import pinsage_ref as PR
from test_pinsage_features_cpu import ProjectorTwin, twin_state_from_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23


def _features(n_items, cards, n_dense, seed):
    from laplace_amd.pinsage.model import ItemFeatures
    g = t.Generator().manual_seed(seed)
    cat = t.stack([t.randint(0, c, (n_items,), generator=g) for c in cards], 1) if cards else None
    dense = t.randn(n_items, n_dense, generator=g) if n_dense else None
    return ItemFeatures(cat.to(DEV) if cat is not None else None, dense.to(DEV) if dense is not None else None,
                        cardinalities=cards if cards else None)


def _twin_of(model, dtype=t.float32):
    """The CPU twin holding the model's projector weights (and features) in `dtype`."""
    pr = model.projector
    tw = ProjectorTwin(model.n_items, model.hidden, pr.cardinalities, 0 if pr.weight is None else pr.weight.shape[1],
                       pr.id_weight is not None, None if pr.x is None else pr.x.cpu(), None if pr.dense is None else pr.dense.cpu())
    with t.no_grad():
        if tw.use_id:
            tw.weight.copy_(pr.id_weight.cpu())
        for a, b in zip(tw.tables, pr.tables):
            a.copy_(b.cpu())
        if tw.n_dense:
            tw.w.copy_(pr.weight.cpu()); tw.b.copy_(pr.bias.cpu())
    return tw.to(dtype)


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------
FWD_CASES = [(4, 1, 0, False), (16, 4, 0, True), (64, 3, 5, False), (128, 16, 512, True)]


@pytest.mark.parametrize("hidden,C,F,use_id", FWD_CASES, ids=["h4c1", "h16c4id", "h64c3f5", "h128c16f512id"])
def test_forward_against_the_twin(hidden, C, F, use_id):
    from laplace_amd.pinsage.model import PinSAGEModel
    I = 1000
    cards = tuple([2, 50, 7, 132, 3, 200, 11, 30, 1, 64, 5, 90, 17, 8, 150, 33][:C])
    t.manual_seed(hidden + C)
    model = PinSAGEModel(I, hidden, 1, features=_features(I, cards, F, 3), use_id=use_id).to(DEV)
    pr = model.projector
    if F:
        with t.no_grad():
            pr.bias.normal_(0, 0.1)
    tw32, tw64 = _twin_of(model), _twin_of(model, t.float64)
    g = t.Generator().manual_seed(5)
    for n in (0, 1, 63, 1000):
        for ids in (t.randint(0, I, (n,), generator=g) // 3 * 3 % I if n else t.zeros(0, dtype=t.int64), None):
            rows = t.arange(n) if ids is None else ids
            with t.no_grad():
                got = pr.project(None, n=n) if ids is None else pr.project(ids.to(DEV))
                assert got.shape == (n, hidden)
                if ids is not None:
                    assert t.equal(pr(ids.to(DEV)), got)                  # the autograd Function's forward is the same call
                if n and F == 0:
                    assert t.equal(got.cpu(), tw32(rows)), (n, ids is None)  # the f32 chain in the documented order, bitwise
                if n:
                    terms = tw64.terms(rows)
                    want = sum(terms)
                    mag = sum(x.abs() for x in terms)
                    if F:      # the dense term's own |products|
                        mag = mag - terms[-1].abs() + tw64.dense[rows].double().abs() @ tw64.w.abs().t() + tw64.b.abs()
                    err = (got.cpu().double() - want).abs()
                    bound = (F + C + 3) * EPS * mag
                    assert bool((err <= bound).all()), (n, ids is None, float((err / bound.clamp(min=1e-300)).max()))


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------
def _check_backward(I, hidden, cards, F, use_id, n, seed, all_items=False):
    from laplace_amd.pinsage.model import PinSAGEModel
    t.manual_seed(seed)
    model = PinSAGEModel(I, hidden, 1, features=_features(I, cards, F, seed), use_id=use_id).to(DEV)
    pr = model.projector
    g = t.Generator().manual_seed(seed + 1)
    ids = None if all_items else t.randint(0, max(I // 2, 1), (n,), generator=g)          # repeats: n draws from I / 2 ids
    rows = t.arange(n) if ids is None else ids
    gout = t.randn(n, hidden, generator=g)
    params = pr.parameter_list()
    SENTINEL = 7.0
    bufs = [t.full_like(p, SENTINEL) for p in params]
    pr.project_backward(None if ids is None else ids.to(DEV), gout.to(DEV), bufs)
    again = [t.full_like(p, SENTINEL) for p in params]
    pr.project_backward(None if ids is None else ids.to(DEV), gout.to(DEV), again)
    assert all(t.equal(a, b) for a, b in zip(bufs, again))                 # no atomics: equal bits
    # float64 autograd of the twin
    tw = _twin_of(model, t.float64)
    tw(rows).backward(gout.double())
    names = (["weight"] if use_id else []) + [f"tables.{c}" for c in range(len(cards))] + (["w", "b"] if F else [])
    want = dict(tw.named_parameters())
    absg = gout.double().abs()
    for name, buf in zip(names, bufs):
        ref, got = want[name].grad, buf.cpu().double()
        if name == "w":       # n products g[r, h] * dense[r, f] per element
            bound = n * EPS * (absg.t() @ tw.dense[rows].double().abs())
        elif name == "b":
            bound = n * EPS * absg.sum(0)
        else:                 # per table row: (run length) * 2^-23 * sum |g| over the run
            codes = rows if name == "weight" else tw.categorical[rows, int(name.split(".")[1])]
            count = t.zeros(ref.shape[0], dtype=t.float64).index_add_(0, codes, t.ones(n, dtype=t.float64))
            sums = t.zeros_like(ref).index_add_(0, codes, absg)
            bound = count[:, None] * EPS * sums
            touched = count > 0
            assert bool((got[~touched] == SENTINEL).all()), name              # rows nobody looks up: left as the caller had them
            got, ref, bound = got[touched], ref[touched], bound[touched]
            if n:
                assert int(count.max()) >= 1
        err = (got - ref).abs()
        assert bool((err <= bound).all()), (name, float(err.max()))
    return model


def test_backward_long_runs_against_float64_autograd():
    """Cardinality 2: two runs of ~1500 references (24 chunks each, combined in chunk order); 50: runs of ~60 that cross chunk
    borders at every offset; 100 000: mostly runs of one.  The id column: runs of the ids' repeats."""
    _check_backward(5000, 32, (2, 50, 100_000), 3, True, 3000, 11)


@pytest.mark.parametrize("n,cards", [(1, (2, 50)), (65, (1, 50)), (0, (2, 50))], ids=["n1", "n65_one_border", "n0"])
def test_backward_small(n, cards):
    """n = 65 with a one-valued column: one run of 65 references, crossing exactly one chunk border."""
    _check_backward(200, 16, cards, 2, False, n, 13 + n)


def test_backward_whole_catalogue_without_ids():
    _check_backward(700, 128, (5, 30), 0, True, 700, 17, all_items=True)


# n = 200, cardinalities (1, 3, 50), ids drawn from 40 items: with the id table 4 slots and 800 references in 13 pieces of 64.
# The one-valued column is one run of 200 over 4 pieces (the two middle ones wholly inside it); the slot borders (200, 400,
# 600) fall inside pieces.  hidden 20: 5 float4 lanes of a group of 8; hidden 128: groups of 32.  n = 65 with one one-valued
# column: exactly one border.
BITS_CASES = [(200, (1, 3, 50), True, 16), (200, (1, 3, 50), False, 16), (200, (1, 3, 50), True, 20), (200, (1, 3, 50), False, 20),
              (200, (1, 3, 50), True, 128), (200, (1, 3, 50), False, 128), (65, (1,), False, 16), (1, (1, 3, 50), True, 16)]


@pytest.mark.parametrize("n,cards,use_id,hidden", BITS_CASES,
                         ids=[f"n{n}c{len(c)}{'id' if u else ''}h{h}" for n, c, u, h in BITS_CASES])
def test_backward_bits_are_the_documented_association(n, cards, use_id, hidden):
    """torch.equal with tests/segsum_emulation.py on every table row; rows nobody looks up keep the sentinel."""
    import segsum_emulation as E
    from laplace_amd.pinsage.model import PinSAGEModel
    I, SENTINEL = 300, 7.0
    t.manual_seed(n + hidden)
    model = PinSAGEModel(I, hidden, 1, features=_features(I, cards, 0, 3), use_id=use_id).to(DEV)
    pr = model.projector
    g = t.Generator().manual_seed(n + 1)
    ids = t.randint(0, 40, (n,), generator=g)                              # repeats: runs in the id slot
    gout = t.randn(n, hidden, generator=g)
    bufs = [t.full_like(p, SENTINEL) for p in pr.parameter_list()]
    pr.project_backward(ids.to(DEV), gout.to(DEV), bufs)
    x = pr.x.cpu()
    slots = [x[ids, c].numpy() for c in range(len(cards))] + ([ids.numpy()] if use_id else [])   # the columns, then the id
    sums = E.segmented_sum(*E.projector_references(slots, gout.numpy()))
    assert len(sums) == sum(len(np.unique(s)) for s in slots)
    tables = bufs[1:] + bufs[:1] if use_id else bufs                      # parameter_list() has the id table first
    for slot, buf in enumerate(tables):
        want = t.from_numpy(E.expected_tables(sums, slot, buf, SENTINEL))
        assert t.equal(buf.cpu(), want), (slot, float((buf.cpu() - want).abs().max()))


# ---- 3. the model's two iterations against PinSAGERef + twin ---------------------------------------------------------------------
def _pin_graph(seed, U, I, E):
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    ei = S.generate(S.SyntheticSpec(U, I, E, seed=seed, deg_min=1, deg_max=60, zipf_s=0.9))
    u, a = ei[0].numpy(), ei[1].numpy()
    return AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, I)


_GRAPH = {}


def _shared_graph():
    if not _GRAPH:
        _GRAPH["g"] = _pin_graph(5, 2500, 800, 40000)
    return _GRAPH["g"]


@pytest.mark.parametrize("use_id", [True, False], ids=["id+features", "features"])
@pytest.mark.parametrize("hidden,layers,walk", [(16, 2, 2), (64, 2, 3)])
def test_featured_iterations_against_the_oracle_twin(hidden, layers, walk, use_id):
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I, SEED, B = 2500, 800, 31, 48
    users, items = _shared_graph()
    ucsr, icsr = PR.Csr(users.ptr, users.idx), PR.Csr(items.ptr, items.idx)
    smp = PinSAGESampler(users, items, U, I, batch_size=B, random_walk_length=walk, num_layers=layers, seed=SEED)
    t.manual_seed(hidden + layers)
    model = PinSAGEModel(I, hidden, layers, features=_features(I, (7, 132, 30, 50), 5, 9), use_id=use_id).to(DEV)
    with t.no_grad():
        model.bias.normal_(0, 0.1)
        model.projector.bias.normal_(0, 0.1)
    for cv in model.convs:
        cv.dropout.p = 0.0
    ref = PR.PinSAGERef(I, hidden, layers)
    ref.proj = _twin_of(model)
    for cv in ref.convs:
        cv.dropout.p = 0.0
    lr = 3e-3
    opt, opt_ref = t.optim.Adam(model.parameters(), lr=lr), t.optim.Adam(ref.parameters(), lr=lr)
    assert NativePinSAGEStep.unsupported_reason(model, opt) is None
    with pytest.raises(ValueError, match="data_parallel"):
        NativePinSAGEStep(model, opt, data_parallel=True)
    probe, full = NativePinSAGEStep(model, opt, keep_grads=True), None
    model.train(); ref.train()
    to_ref = {k: k2 for k, k2 in zip(model.state_dict().keys(), twin_state_from_model(model).keys())}
    ref_params = dict(ref.named_parameters())
    assert sorted(to_ref.values()) == sorted(ref_params)

    def compare_grads(what, step, grads_ref):
        for n, p in model.named_parameters():
            g = grads_ref[to_ref[n]]
            scale = float(g.abs().max()) + 1e-12
            assert float((p.grad.cpu() - g).abs().max()) <= 2e-4 * scale + 1e-8, (what, step, n)

    for step in range(3):
        ref.load_state_dict(twin_state_from_model(model))
        got = smp.sample_batch(step)
        wh, wt, wn = PR.item_pairs(B, I, icsr, ucsr, SEED, step)
        want = PR.sample_from_item_pairs(wh, wt, wn, icsr, ucsr, layers, walk, 0.5, 10, 3, SEED, step)
        assert np.array_equal(got["seeds"].cpu().numpy(), want["seeds"])
        opt_ref.zero_grad()
        lb = ref(t.from_numpy(want["seeds"]), tuple(t.from_numpy(x) for x in want["pos"]),
                 tuple(t.from_numpy(x) for x in want["neg"]), PR.to_torch_blocks(want["blocks"])).mean()
        lb.backward()
        grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
        # (a) the autograd path
        opt.zero_grad(set_to_none=True)
        la = model(got["seeds"], got["pos"], got["neg"], got["blocks"]).mean()
        la.backward()
        assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), ("autograd", step)
        compare_grads("autograd", step, grads_ref)
        for p in model.parameters():
            p.grad.zero_()
        # (b) the executor, gradients only
        la = probe.step(got)
        assert la is not None, probe.declined
        assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), ("native", step)
        compare_grads("native", step, grads_ref)
        for p in model.parameters():
            p.grad.zero_()                                                 # what the probe left behind
        # (c) the full iteration from the same weights
        before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        if full is None:
            full = NativePinSAGEStep(model, opt)
        assert full.step(got) is not None, full.declined
        opt_ref.step()
        for n, p in model.named_parameters():
            q, g, b = ref_params[to_ref[n]], grads_ref[to_ref[n]], before[n]
            big = g.abs() > 1e-3 * (float(g.abs().max()) + 1e-12) + 1e-7
            assert bool(big.any()), n
            assert t.allclose((p.detach().cpu() - b)[big], (q.detach() - b)[big], rtol=5e-2, atol=2e-6), (step, n)
            assert t.equal(p.detach().cpu()[g == 0], b[g == 0]) or step > 0   # rows never touched do not move on the first step
            assert float(opt.state[p]["step"]) == step + 1 == float(opt_ref.state[q]["step"])
        # the table gradients (and the scorer bias's) are all-zero again
        for p in [model.bias] + model.projector.parameter_list()[: (1 if use_id else 0) + 4]:
            assert float(p.grad.abs().max()) == 0.0


# ---- 4. catalogue pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_id", [True, False], ids=["id+features", "features"])
def test_featured_catalogue_pass(use_id):
    from laplace_amd.pinsage.model import PinSAGEModel, train_epoch
    from laplace_amd.pinsage.native import embed_items
    from laplace_amd.pinsage.sampler import PinSAGESampler
    from test_gpu_pinsage_eval import _graph
    U, I = 1500, 700
    users, items = _graph(7, U, 600, I, 20000)
    smp = PinSAGESampler(users, items, U, I, batch_size=32, random_walk_length=2, num_layers=2, seed=11)
    t.manual_seed(0)
    model = PinSAGEModel(I, 16, 2, features=_features(I, (7, 132, 30, 50), 5, 4), use_id=use_id).to(DEV)
    opt = t.optim.Adam(model.parameters(), lr=3e-3)
    losses = train_epoch(model, opt, smp, 10)
    assert len(losses) == 10 and all(np.isfinite(losses))
    step = smp.step
    with t.no_grad():
        assert embed_items(model, smp, step) is not None
    h = model.item_representations(smp)
    assert h.shape == (I, 16) and model.training
    model.eval()
    with t.no_grad():
        ref = model.batched_item_representations(smp, step, 97)
    model.train()
    assert float((h - ref).abs().max()) <= 1e-5
    assert t.equal(model.item_representations(smp, step=5), model.item_representations(smp, step=5))


# ---- 5. cold items --------------------------------------------------------------------------------------------------------------------
def test_cold_items_are_placed_by_their_features():
    """600 users, 400 items, 12 000 edges, 8 planted communities (mix 0.85); the item features are generate_hetero's with
    feature_signal: three categorical columns (132, 30, 50 values), the first holding the community, the others noise.  40 items
    lose every edge before training.  Score: the share of a cold item's 10 nearest warm items (dot product of the
    representations) that lie in its community; chance = 1/8.  The CPU twin of this recipe measured 0.12 (id only), 0.96
    (features only), 0.91 (id + features)."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel, train_epoch
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I, K = 600, 400, 8
    spec = S.SyntheticSpec(U, I, 12000, seed=3, communities=K, community_mix=0.85)
    ei = S.generate(spec)
    community = S.item_community(spec)
    rng = np.random.default_rng(1)
    cards = (132, 30, 50)
    x = np.stack([rng.integers(0, c, size=I) for c in cards], 1)
    x[:, 0] = community
    cold = rng.choice(I, 40, replace=False)
    is_cold = np.zeros(I, dtype=bool)
    is_cold[cold] = True
    u, a = ei[0].numpy(), ei[1].numpy()
    keep = ~is_cold[a]
    users, items = AdjList.from_edges(u[keep], a[keep], U), AdjList.from_edges(a[keep], u[keep], I)
    assert all(items.ptr[i + 1] == items.ptr[i] for i in cold)
    feats = ItemFeatures(t.from_numpy(x.astype(np.int64)).to(DEV), cardinalities=cards)
    warm = t.from_numpy(np.flatnonzero(~is_cold)).to(DEV)
    comm = t.from_numpy(community.astype(np.int64)).to(DEV)
    cold_t = t.from_numpy(np.sort(cold)).to(DEV)
    score = {}
    for kind, kw in (("id", dict()), ("features", dict(features=feats, use_id=False)), ("id+features", dict(features=feats))):
        t.manual_seed(0)
        model = PinSAGEModel(I, 32, 2, **kw).to(DEV)
        smp = PinSAGESampler(users, items, U, I, batch_size=32, random_walk_length=2, num_random_walks=10, num_neighbors=3,
                             num_layers=2, seed=5)
        opt = t.optim.Adam(model.parameters(), lr=3e-3)
        train_epoch(model, opt, smp, 300)
        h = model.item_representations(smp)
        near = (h[cold_t] @ h[warm].t()).topk(10, dim=1).indices
        score[kind] = float((comm[warm][near] == comm[cold_t][:, None]).float().mean())
    chance = 1.0 / K
    print(f"cold items, same-community share of the 10 nearest warm items: id {score['id']:.3f}, "
          f"features {score['features']:.3f}, id+features {score['id+features']:.3f} (chance {chance:.3f})")
    assert score["id"] <= 2 * chance
    assert score["features"] >= 4 * chance and score["features"] > score["id"]
    assert score["id+features"] >= 4 * chance and score["id+features"] > score["id"]
