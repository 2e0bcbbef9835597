"""GPU: the full-catalogue softmax (mi_full_softmax_fwd_bwd_f32) against its float64 twin (tests/full_softmax_twin.py) on
the shared cases, its lane maps on exact-integer data, its scales, its loss-only form and determinism, the M-negative and the
in-batch kernels it coincides with on small catalogues, its refusals, the autograd function, the trainer with
full_softmax=True, the pipeline, and a quality floor.

Tolerances are the project's (tests/test_gpu_lightgcn.py): loss 1e-6 * max(1, |loss|), gradients atol 1e-6 / rtol 1e-4,
trained embeddings <= 1e-4.

Measured maxima on an MI355X are in profiles/full_softmax.md."""
import json
import math
import os
import sys

import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_softmax_twin as T  # noqa: E402
from oracle import lightgcn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAMS = (0.0, 1e-2)


def _ops():
    from laplace_amd import ops
    return ops


def _loss_close(got, want):
    return abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


def _device_call(c, lam, g_scale=1.0, reg_scale=1.0, want_grad=True):
    """(loss, dL/dfinal [U + I, d] or None, reg_w or None) of case c from the kernel."""
    U, I, d = c["U"], c["I"], c["d"]
    gf = t.zeros(U + I, d, device=DEV) if want_grad else None
    reg_w = t.zeros(U + I, device=DEV) if want_grad else None
    loss = _ops().full_softmax_fwd_bwd(c["users"].to(DEV), c["pos"].to(DEV), c["final"].to(DEV), c["e0"].to(DEV), U, lam,
                                       g_final=gf, reg_w=reg_w, g_scale=g_scale, reg_scale=reg_scale)
    return loss, gf, reg_w


# ---------------------------------------------------------------------------- 1: kernel vs the float64 twin
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_kernel_matches_float64_twin(i, lam):
    c = T.cases()[i]
    U, I = c["U"], c["I"]
    want, g_fin, g_e0 = T.reference(i, lam)
    ops = _ops()
    # the item rows start as NaN here: the kernel stores every one of them, so none survives (the user rows start at zero, as
    # the contract has it: the batch does not name them all)
    gf = t.zeros(U + I, c["d"], device=DEV)
    gf[U:] = float("nan")
    reg_w = t.zeros(U + I, device=DEV)
    loss = ops.full_softmax_fwd_bwd(c["users"].to(DEV), c["pos"].to(DEV), c["final"].to(DEV), c["e0"].to(DEV), U, lam,
                                    g_final=gf, reg_w=reg_w)
    got_e0 = (reg_w[:, None].cpu() * c["e0"]).double()
    print(f"case {i} B={c['B']} d={c['d']} I={I} lam={lam}: loss {float(loss):.9f} want {float(want):.9f} |dloss| "
          f"{abs(float(loss) - float(want)):.3e} max |dg| {float((gf.cpu().double() - g_fin).abs().max()):.3e} "
          f"max |dreg| {float((got_e0 - g_e0).abs().max()):.3e}")
    assert not bool(t.isnan(gf).any())                       # every item row was stored
    assert _loss_close(loss, want)
    assert t.allclose(gf.cpu().double(), g_fin, atol=1e-6, rtol=1e-4)
    assert t.allclose(got_e0, g_e0, atol=1e-6, rtol=1e-4)
    # user rows the batch does not name stay exactly zero, in the kernel and in the twin
    idle = t.ones(U, dtype=t.bool)
    idle[c["users"]] = False
    assert float(gf.cpu()[:U][idle].abs().sum()) == 0.0 and float(g_fin[:U][idle].abs().sum()) == 0.0
    touched = ~t.cat([idle, t.ones(I, dtype=t.bool)])
    touched[U + c["pos"]] = True
    assert float(reg_w.cpu()[~touched].abs().sum()) == 0.0
    if I == 1:                                               # main term exactly 0, gradients exactly 0
        assert float(gf.abs().max()) == 0.0
        if lam == 0.0:
            assert float(loss) == 0.0


# ---------------------------------------------------------------------------- 2: lane maps
@pytest.mark.parametrize("d", [64, 100])
def test_lane_maps_with_exact_integer_asymmetric_data(d):
    """Small-integer rows whose softmax saturates, on a catalogue that is no multiple of 32 (B = 64, I = 80): slot b's logit
    for item s(b) = (7b + 3) mod 80 (injective, 7 and 80 coprime) lies some 4000 above the others, so in fp32 exp gives
    exactly 1 for it and 0 for the rest; with pos_b = (s(b) + 40) mod 80 the coefficients are exactly +1 at (b, s(b)) and -1
    at (b, pos_b) (g_scale = B), and both gradients are small-integer sums: exact whatever the order, so a lane, row, tile
    or chunk mix-up in either sweep shows as a wrong integer."""
    B, I = 64, 80
    g = t.Generator().manual_seed(d)
    b = t.arange(B)
    s = (7 * b + 3) % I
    pos = (s + 40) % I
    Uu = t.randint(-1, 2, (B, d), generator=g).float()
    V = t.randint(-1, 2, (I, d), generator=g).float()
    Uu[b, b % d] += 64.0
    V[s, b % d] += 64.0                                      # <u_b, v_s(b)> ~ 4096; every other pair at most a few hundred
    C = t.zeros(B, I)
    C[b, s] = 1.0
    C[b, pos] -= 1.0
    logit = Uu @ V.T                                         # integers below 2^24: exact in fp32
    planted = t.zeros(B, I, dtype=t.bool)
    planted[b, s] = True
    assert float(logit[~planted].abs().max()) < 1000 and float(logit[planted].min()) > 3500
    # the construction is exact in fp32 on the CPU: lse is the planted logit itself, the softmax a one-hot row
    lse = t.logsumexp(logit, dim=1)
    assert t.equal(lse, logit[b, s]) and t.equal(t.exp(logit - lse[:, None]), planted.float())
    want = t.cat([C @ V, C.T @ Uu])
    final = t.cat([Uu, V]).to(DEV)
    gf = t.zeros(B + I, d, device=DEV)
    _ops().full_softmax_fwd_bwd(b.to(DEV), pos.to(DEV), final, final, B, 0.0, g_final=gf, g_scale=float(B))
    assert t.equal(gf.cpu(), want)


# ---------------------------------------------------------------------------- 3: scales
@pytest.mark.parametrize("i", [0, 3, 4, 5])
def test_gradient_scale_and_reg_scale(i):
    c = T.cases()[i]
    lam = 1e-2
    want, g_fin, g_e0 = T.reference(i, lam)
    loss, gf, reg_w = _device_call(c, lam, g_scale=0.25, reg_scale=0.5)
    assert _loss_close(loss, want)                       # neither scale touches the loss value
    assert t.allclose(gf.cpu().double(), 0.25 * g_fin, atol=1e-6, rtol=1e-4)
    assert t.allclose((reg_w[:, None].cpu() * c["e0"]).double(), 0.5 * g_e0, atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 4: loss-only form, determinism
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_loss_only_form_and_second_call_give_equal_bits(i):
    c = T.cases()[i]
    a = _device_call(c, 1e-2)
    b = _device_call(c, 1e-2)
    assert t.equal(a[0], b[0]) and t.equal(a[1], b[1]) and t.equal(a[2], b[2])
    only = _device_call(c, 1e-2, want_grad=False)
    assert t.equal(only[0], a[0])
    assert float(a[1].abs().max()) > 0.0 or c["I"] == 1


def _loss_bits_tool():
    """tools/record_loss_bits.py: the cases of tests/golden/tile_loss_bits.json and the function that records one."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_loss_bits
    return record_loss_bits


@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_every_shape_gives_its_recorded_bits(i):
    """Loss, g_final, reg_w and the loss-only form's loss of every shape of the twin over lam in LAMS at g_scale = 1/3,
    against the bits recorded at the commit tests/golden/tile_loss_bits.json names.  The cases and the recording are the
    tool's: neither side changes alone."""
    tool = _loss_bits_tool()
    assert tool.FULL_LAMS == LAMS and tool.full_softmax_shapes() == len(T.SHAPES)
    with open(os.path.join(ROOT, "tests", "golden", "tile_loss_bits.json")) as f:
        rec = json.load(f)["full_softmax"]
    assert len(rec) == len(LAMS) * len(T.SHAPES)
    for c in tool.full_softmax_cases(i):
        assert tool.full_softmax_record(c) == rec[c["key"]], c["key"]


# ---------------------------------------------------------------------------- 5: against the other softmax kernels
def test_seventeen_items_equal_the_sampled_softmax_kernel_over_the_sixteen_others():
    ops = _ops()
    c = T.cases()[1]
    B, U, I, d, lam = c["B"], c["U"], c["I"], c["d"], 1e-2
    assert B == 17 and I == 17
    loss, gf, _ = _device_call(c, lam)
    neg = t.tensor([[i for i in range(I) if i != p] for p in c["pos"].tolist()])   # [17, 16]: every other item
    g2, rw2 = t.zeros(U + I, d, device=DEV), t.zeros(U + I, device=DEV)
    # lambda = 0 there and the L2 term apart: the M-negative loss also counts the rows of its negatives
    loss2 = ops.rank_loss_fwd_bwd(c["users"].to(DEV), c["pos"].to(DEV), neg.to(DEV), c["final"].to(DEV), c["e0"].to(DEV), U,
                                  0.0, objective="softmax", g_final=g2, reg_w=rw2)
    l2 = lam * (c["e0"][c["users"]].double().pow(2).sum() + c["e0"][U + c["pos"]].double().pow(2).sum())
    print(f"full {float(loss):.9f}, M = 16 kernel + L2 {float(loss2) + float(l2):.9f}, max |dg| {float((gf - g2).abs().max()):.3e}")
    assert _loss_close(loss, float(loss2) + float(l2))
    assert t.allclose(gf, g2, atol=1e-6, rtol=1e-4)


def test_a_permutation_batch_equals_the_in_batch_kernel_over_one_group():
    """B = I = 64, pos a permutation and the users distinct: the positives of the one group ARE the catalogue, nothing is masked."""
    ops = _ops()
    B, d, lam = 64, 32, 1e-2
    g = t.Generator().manual_seed(77)
    final, e0 = (0.3 * t.randn(2 * B, d, generator=g)).to(DEV), t.randn(2 * B, d, generator=g).to(DEV)
    users, pos = t.randperm(B, generator=g).to(DEV), t.randperm(B, generator=g).to(DEV)
    out = []
    for call in (lambda **kw: ops.full_softmax_fwd_bwd(users, pos, final, e0, B, lam, **kw),
                 lambda **kw: ops.inbatch_softmax_fwd_bwd(users, pos, final, e0, B, lam, group=64, logq=None, **kw)):
        gf, rw = t.zeros(2 * B, d, device=DEV), t.zeros(2 * B, device=DEV)
        out.append((call(g_final=gf, reg_w=rw).clone(), gf, rw))
    (la, ga, ra), (lb, gb, rb) = out
    print(f"full {float(la):.9f}, in-batch {float(lb):.9f}, max |dg| {float((ga - gb).abs().max()):.3e}")
    assert _loss_close(la, lb) and t.allclose(ga, gb, atol=1e-6, rtol=1e-4) and t.equal(ra, rb)


# ---------------------------------------------------------------------------- 6: refusals
def test_refusals():
    ops = _ops()
    from laplace_amd._lib import MiError
    u, p = t.zeros(64, dtype=t.int64, device=DEV), t.zeros(64, dtype=t.int64, device=DEV)
    for d in (260, 30):
        with pytest.raises((MiError, ValueError)):
            ops.full_softmax_fwd_bwd(u, p, t.zeros(9, d, device=DEV), t.zeros(9, d, device=DEV), 4, 1e-6)
    with pytest.raises(MiError):
        ops.full_softmax_fwd_bwd(u.cpu(), p.cpu(), t.zeros(9, 32), t.zeros(9, 32), 4, 1e-6)
    with pytest.raises((MiError, ValueError)):       # g_final must hold every item row
        ops.full_softmax_fwd_bwd(u, p, t.zeros(9, 32, device=DEV), t.zeros(9, 32, device=DEV), 4, 1e-6,
                                 g_final=t.zeros(8, 32, device=DEV))
    # the library's own answers, past the Python checks
    from laplace_amd import _lib
    L = _lib.lib()
    x, out = t.zeros(9, 260, device=DEV), t.zeros(1, device=DEV)
    ws = t.zeros(L.mi_full_softmax_workspace_bytes(64, 32, 5), dtype=t.uint8, device=DEV)

    def raw(d, n_items=5, reg_w=None, ws_bytes=ws.numel()):
        return L.mi_full_softmax_fwd_bwd_f32(64, d, 4, n_items, u.data_ptr(), p.data_ptr(), x.data_ptr(), 260, x.data_ptr(),
                                             260, 1e-6, 1.0, 1.0, out.data_ptr(), None, 0, reg_w, ws.data_ptr(), ws_bytes,
                                             None)
    assert raw(260) == _lib.MI_ERR_UNSUPPORTED and raw(30) == _lib.MI_ERR_UNSUPPORTED
    assert raw(32, reg_w=out.data_ptr()) == _lib.MI_ERR_UNSUPPORTED and raw(32, n_items=0) == _lib.MI_ERR_BAD_ARG
    assert raw(32, ws_bytes=ws.numel() - 1) == _lib.MI_ERR_WORKSPACE and raw(32) == 0


# ---------------------------------------------------------------------------- 7: autograd function
def test_autograd_function_against_the_twin():
    from laplace_amd.utils.metrics_lightgcn import full_softmax_loss
    c = T.cases()[3]                                     # 5 users, 6 items: every id repeats
    U, lam = c["U"], 1e-2
    users, pos = c["users"], c["pos"]
    want, g_fin, g_e0 = T.reference(3, lam)
    f = c["final"].to(DEV).requires_grad_(True)
    e = c["e0"].to(DEV).requires_grad_(True)
    ud, pd = users.to(DEV), pos.to(DEV)
    loss = full_softmax_loss(f[ud], f[U:], pd, e[ud], e[U + pd], lam)
    (2.0 * loss).backward()
    assert _loss_close(loss.detach(), want)
    assert t.allclose(f.grad.cpu().double(), 2.0 * g_fin, atol=2e-6, rtol=1e-4)
    assert t.allclose(e.grad.cpu().double(), 2.0 * g_e0, atol=2e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 8: trainer
def _model_and_graph(U, I, n_edges, D, K, seed):
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    g = t.Generator().manual_seed(seed)
    ei = t.stack([t.randint(0, U, (n_edges,), generator=g), t.randint(0, I, (n_edges,), generator=g)])
    t.manual_seed(seed)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K)
    inter = Interactions(ei, U, I)
    return model, inter, inter.adjacency("bipartite"), ei


GRAPH = dict(U=400, I=300, n_edges=6000, D=64, K=3, seed=23)     # those of tests/test_gpu_inbatch_softmax.py
B_TRAIN, LAM_TRAIN, STEPS = 160, 1e-5, 6
FULL = dict(full_softmax=True, sparse_batch=False)


def _trainer(**kw):
    from laplace_amd.trainer import LightGCNTrainer
    model, inter, adj, _ = _model_and_graph(**GRAPH)
    model.to(DEV)
    return model, LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), lr=1e-3, Lambda=LAM_TRAIN, batch_size=B_TRAIN, seed=5,
                                  objective="softmax", **kw)


def _run(batches=None, **kw):
    model, tr = _trainer(**kw)
    losses, used = [], []
    for i in range(STEPS):
        batch = batches[i] if batches is not None else tuple(x.clone() for x in tr.sample())
        used.append(batch)
        losses.append(float(tr.step(batch)))
    tr.finish()
    return losses, used, tr.table.clone(), tr


@pytest.fixture(scope="module")
def autograd_run():
    """Six steps of torch fp32 autograd over the twin with torch.optim.Adam, on the batches the uniform sampler draws at
    seed 5, and a negatives="uniform" run made BEFORE any full-softmax trainer exists."""
    uniform_before = _run(negatives="uniform", n_neg=1)
    model, inter, adj, _ = _model_and_graph(**GRAPH)
    U, K = GRAPH["U"], GRAPH["K"]
    uw = t.nn.Parameter(model.users_emb.weight.detach().clone())
    iw = t.nn.Parameter(model.items_emb.weight.detach().clone())
    opt = t.optim.Adam([uw, iw], lr=1e-3)
    row, col, _ = adj.coo()
    batches, losses = [], []
    for users, pos, _neg in uniform_before[1]:
        uf, u0, itf, it0 = R.lightgcn_forward(uw, iw, row, col, K)
        want = T.twin_loss(t.cat([uf, itf]), t.cat([u0, it0]), U, users.cpu(), pos.cpu(), LAM_TRAIN)
        opt.zero_grad()
        want.backward()
        opt.step()
        batches.append((users, pos))
        losses.append(float(want))
    return dict(batches=batches, losses=losses, uw=uw.detach(), iw=iw.detach(), uniform_before=uniform_before)


@pytest.mark.parametrize("reorder", [False, True])
def test_trainer_six_steps_match_autograd_loop(autograd_run, reorder):
    ref = autograd_run
    losses, _, table, tr = _run(batches=ref["batches"], reorder=reorder, **FULL)
    assert tr.full_softmax and tr.in_batch and tr.logq is None and not tr.logq_correction and tr.in_batch_group is None
    assert (tr.order is not None) == reorder
    U = GRAPH["U"]
    du = float((table[:U].cpu() - ref["uw"]).abs().max())
    di = float((table[U:].cpu() - ref["iw"]).abs().max())
    print(f"reorder={reorder}: max |dloss| {max(abs(a - b) for a, b in zip(losses, ref['losses'])):.3e}, "
          f"max |dtable| {max(du, di):.3e}")
    for a, b in zip(losses, ref["losses"]):
        assert _loss_close(a, b)
    assert du <= 1e-4 and di <= 1e-4
    # bitwise reproducible, and a 3-tuple's third entry is ignored
    junk = [(u, p, t.zeros_like(p)) for u, p in ref["batches"]]
    again = _run(batches=junk, reorder=reorder, **FULL)
    assert again[0] == losses and t.equal(again[2], table)


def test_trainer_draws_the_uniform_edge_stream_and_leaks_no_state(autograd_run):
    ref = autograd_run
    before = ref["uniform_before"]
    own = _run(**FULL)                                    # the full-softmax trainer's own batches
    for (u, p, _), (u2, p2, _) in zip(own[1], before[1]):
        assert t.equal(u, u2) and t.equal(p, p2)
    given = _run(batches=ref["batches"], **FULL)
    assert own[0] == given[0] and t.equal(own[2], given[2])
    after = _run(negatives="uniform", n_neg=1)            # a uniform trainer after the full-softmax ones: as before them
    assert after[0] == before[0] and t.equal(after[2], before[2])
    assert not after[3].full_softmax and not after[3].in_batch
    assert max(abs(a - b) for a, b in zip(own[0], before[0])) > 1e-3     # and it is another objective


# ---------------------------------------------------------------------------- 9: pipeline
def test_pipeline_passes_the_full_softmax_through(tmp_path):
    """run_pipeline_lightgcn.train under compat="reference", whose negative range and sampler quirk the full softmax leaves
    out: the run ends with finite statistics, and its training loss is not the in-batch run's."""
    from dataclasses import replace
    from laplace_amd.config import lightgcn_config
    from laplace_amd.run_pipeline_lightgcn import train
    from test_gpu_acceptance import _tastes_graph
    cfg = replace(lightgcn_config, epochs=30, k=12, hidden_layer_size=32, learning_rate=1e-3, save_model=False, batch_size=128,
                  num_iterations=2, eval_every=100, lr_decay_every=100, Lambda=1e-6, show_graph=False, num_recommendations=64)
    ei = t.from_numpy(_tastes_graph(300, 200, 1000, seed=42).T.copy())
    out = {}
    for name, kw in (("full", dict(full_softmax=True)), ("in_batch", dict(negatives="in_batch", in_batch_group=128))):
        t.manual_seed(42)
        stats = train(cfg, edge_index=ei, num_users=300, num_articles=200, compat="reference", device=DEV, seed=42,
                      verbose=False, save_dir=str(tmp_path / name), objective="softmax", predictor="propagated", **kw)
        for v in (stats.loss, stats.recall_val, stats.recall_test, stats.precision_val, stats.precision_test):
            assert math.isfinite(v)
        out[name] = stats.loss
    assert out["full"] != out["in_batch"]
    with pytest.raises(ValueError):
        train(cfg, edge_index=ei, num_users=300, num_articles=200, device=DEV, verbose=False, objective="bpr", full_softmax=True)


# ---------------------------------------------------------------------------- 10: quality floor
def test_full_softmax_beats_the_popularity_predictor():
    """The `worth` recipe of tools/bench_inbatch.py (that of profiles/neg_sampling.md section 4: C1-scale planted graph, spec
    seed 5, D 64, K 2, batch 1024, lr 1e-2, lambda 1e-6, 200 steps, bench.map_at_12) at trainer seed 7: the propagated MAP@12
    must reach the popularity predictor's, scored in the same call."""
    import bench
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    spec = S.SyntheticSpec(num_users=S.C1.num_users, num_items=S.C1.num_items, num_edges=S.C1.num_edges, seed=5,
                           communities=8, community_mix=0.85, deg_min=1, deg_max=S.C1.num_items // 2)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).to(DEV)
    inter = Interactions(ei.to(DEV), spec.num_users, spec.num_items)
    t.manual_seed(0)
    model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
    tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024, seed=7,
                         objective="softmax", **FULL)
    got = bench.map_at_12(model, tr, inter, held, 200)
    print("full softmax: propagated MAP@12", got["propagated_embeddings_map_at_12"], "layer-0", got["value"],
          "popularity", got["popularity_predictor_map_at_12"], "loss", float(tr.loss))
    assert got["propagated_embeddings_map_at_12"] >= got["popularity_predictor_map_at_12"]
