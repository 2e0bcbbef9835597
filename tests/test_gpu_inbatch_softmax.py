"""GPU: the in-batch sampled softmax (mi_inbatch_softmax_fwd_bwd_f32) against its float64 twin
(tests/inbatch_softmax_twin.py) on the shared cases, its loss-only form, its determinism, the M-negative kernel it reduces
to on distinct ids, its refusals, the trainer with negatives="in_batch" in every step form, and a quality floor.

Tolerances are the project's (tests/test_gpu_lightgcn.py): loss 1e-6 * max(1, |loss|), gradients atol 1e-6 / rtol 1e-4,
trained embeddings <= 1e-4.

Measured maxima on an MI355X are in profiles/inbatch_softmax.md, section (e)."""
import json
import os
import sys

import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inbatch_softmax_twin as T  # noqa: E402
from oracle import lightgcn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAMS = (0.0, 1e-2)


def _ops():
    from laplace_amd import ops
    return ops


def _loss_close(got, want):
    return abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


def _device_call(c, lam, logq, with_map, g_scale=1.0, reg_scale=1.0, want_grad=True):
    """(loss, dL/dfinal [U + I, d] or None, reg_w or None) of case c from the kernel, through a compact table or not."""
    ops = _ops()
    U, I, d, B = c["U"], c["I"], c["d"], c["B"]
    ud, pd = c["users"].to(DEV), c["pos"].to(DEV)
    lq = None if logq is None else logq.to(DEV)
    final, e0 = c["final"].to(DEV), c["e0"].to(DEV)
    reg_w = t.zeros(U + I, device=DEV) if want_grad else None
    kw = dict(group=c["G"], logq=lq, reg_w=reg_w, g_scale=g_scale, reg_scale=reg_scale)
    if not with_map:
        gf = t.zeros(U + I, d, device=DEV) if want_grad else None
        loss = ops.inbatch_softmax_fwd_bwd(ud, pd, final, e0, U, lam, g_final=gf, **kw)
        return loss, gf, reg_w
    gmap, nodes, cnt = ops.batch_nodes(ud, pd, pd, U, U + I)      # the node set of (users, pos): neg aliased to pos
    n = int(cnt[0])
    rows = nodes[:n].long()
    compact = t.zeros(2 * B, d, device=DEV)
    compact[:n] = final[rows]
    gc = t.zeros(2 * B, d, device=DEV) if want_grad else None
    loss = ops.inbatch_softmax_fwd_bwd(ud, pd, compact, e0, U, lam, g_final=gc, node_map=gmap, **kw)
    if not want_grad:
        return loss, None, None
    assert float(gc[n:].abs().max()) == 0.0 if n < 2 * B else True   # rows beyond the count stay zero
    gf = t.zeros(U + I, d, device=DEV)
    gf[rows] = gc[:n]
    return loss, gf, reg_w


# ---------------------------------------------------------------------------- 1: kernel vs the float64 twin
@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("with_logq", [False, True])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_kernel_matches_float64_twin(i, lam, with_logq, with_map):
    c = T.cases()[i]
    want, g_fin, g_e0 = T.reference(i, lam, with_logq)
    loss, gf, reg_w = _device_call(c, lam, c["logq"] if with_logq else None, with_map)
    got_e0 = (reg_w[:, None].cpu() * c["e0"]).double()
    print(f"case {i} B={c['B']} G={c['G']} d={c['d']} lam={lam} logq={with_logq} map={with_map}: loss {float(loss):.9f} "
          f"want {float(want):.9f} |dloss| {abs(float(loss) - float(want)):.3e} max |dg| "
          f"{float((gf.cpu().double() - g_fin).abs().max()):.3e} max |dreg| {float((got_e0 - g_e0).abs().max()):.3e}")
    assert _loss_close(loss, want)
    assert t.allclose(gf.cpu().double(), g_fin, atol=1e-6, rtol=1e-4)
    assert t.allclose(got_e0, g_e0, atol=1e-6, rtol=1e-4)
    # rows the batch does not touch stay zero
    touched = t.zeros(c["U"] + c["I"], dtype=t.bool)
    touched[c["users"]] = True
    touched[c["U"] + c["pos"]] = True
    assert float(gf.cpu()[~touched].abs().sum()) == 0.0 and float(reg_w.cpu()[~touched].abs().sum()) == 0.0


@pytest.mark.parametrize("d", [64, 100])
def test_lane_maps_with_exact_integer_asymmetric_data(d):
    """Small-integer rows whose softmax saturates: slot b's logit for candidate s(b) = (5b + 3) mod 64 (a permutation without
    fixed point or symmetry) lies some 4000 above the others, so in fp32 exp gives exactly 1 for it and 0 for the rest, the
    coefficients are exactly +1 at (b, s(b)) and -1 at (b, b) (g_scale = B), and both gradients are small-integer sums:
    exact whatever the order, so a lane, row or tile mix-up in either sweep shows as a wrong integer."""
    ops = _ops()
    B = 64                                                  # one group of two tiles a side
    g = t.Generator().manual_seed(d)
    s = (5 * t.arange(B) + 3) % B
    U = t.randint(-1, 2, (B, d), generator=g).float()
    V = t.randint(-1, 2, (B, d), generator=g).float()
    U[t.arange(B), t.arange(B) % d] += 64.0
    V[s, t.arange(B) % d] += 64.0                           # <u_b, v_s(b)> ~ 4096; every other pair at most a few hundred
    C = t.zeros(B, B)
    C[t.arange(B), s] = 1.0
    C[t.arange(B), t.arange(B)] -= 1.0
    assert float(((U @ V.T) * (1 - C.abs())).abs().max()) < 1000 and float((U @ V.T)[t.arange(B), s].min()) > 3500
    want = t.cat([C @ V, C.T @ U])
    a = t.arange(B, device=DEV)
    final = t.cat([U, V]).to(DEV)
    gf = t.zeros(2 * B, d, device=DEV)
    ops.inbatch_softmax_fwd_bwd(a, a, final, final, B, 0.0, group=64, g_final=gf, g_scale=float(B))
    assert t.equal(gf.cpu(), want)


@pytest.mark.parametrize("i", [0, 3, 4, 6])
def test_gradient_scale_and_reg_scale(i):
    c = T.cases()[i]
    lam = 1e-2
    want, g_fin, g_e0 = T.reference(i, lam, True)
    loss, gf, reg_w = _device_call(c, lam, c["logq"], False, g_scale=0.25, reg_scale=0.5)
    assert _loss_close(loss, want)                       # neither scale touches the loss value
    assert t.allclose(gf.cpu().double(), 0.25 * g_fin, atol=1e-6, rtol=1e-4)
    assert t.allclose((reg_w[:, None].cpu() * c["e0"]).double(), 0.5 * g_e0, atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 2, 3: loss-only form, determinism
@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_loss_only_form_and_second_call_give_equal_bits(i, with_map):
    c = T.cases()[i]
    a = _device_call(c, 1e-2, c["logq"], with_map)
    b = _device_call(c, 1e-2, c["logq"], with_map)
    assert t.equal(a[0], b[0]) and t.equal(a[1], b[1]) and t.equal(a[2], b[2])
    only = _device_call(c, 1e-2, c["logq"], with_map, want_grad=False)
    assert t.equal(only[0], a[0])
    assert float(a[1].abs().max()) > 0.0


def _loss_bits_tool():
    """tools/record_loss_bits.py: the cases of tests/golden/loss_path_bits.json and the function that records one."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_loss_bits
    return record_loss_bits


@pytest.mark.parametrize("i", range(len(T.SHAPES) + 2))
def test_every_shape_gives_its_recorded_bits(i):
    """Loss, g_final, reg_w and the loss-only form's loss of every shape of the twin, and of B = 32 and B = 33 at G = 32 (64
    sorted references: one full chunk; and one reference more), over lam in LAMS, logq off and on, node map off and on,
    against the bits recorded at the commit tests/golden/loss_path_bits.json names.  The cases and the recording are the
    tool's: neither side changes alone."""
    tool = _loss_bits_tool()
    assert tool.INBATCH_LAMS == LAMS and tool.inbatch_shapes() == len(T.SHAPES) + 2
    with open(os.path.join(ROOT, "tests", "golden", "loss_path_bits.json")) as f:
        rec = json.load(f)["in_batch"]
    assert len(rec) == 8 * tool.inbatch_shapes()
    for c in tool.inbatch_cases(i):
        assert tool.inbatch_record(c) == rec[c["key"]], c["key"]


# ---------------------------------------------------------------------------- 4: against the M-negative kernel
@pytest.mark.parametrize("with_logq", [False, True])
def test_distinct_ids_equal_the_sampled_softmax_kernel_over_the_other_positives(with_logq):
    ops = _ops()
    c = T.cases()[1]
    B, U, I, d, lam = c["B"], c["U"], c["I"], c["d"], 1e-2
    assert B == 17 and len(set(c["users"].tolist())) == B and len(set(c["pos"].tolist())) == B
    logq = c["logq"] if with_logq else None
    loss, gf, reg_w = _device_call(c, lam, logq, False)
    others = t.tensor([[j for j in range(B) if j != b] for b in range(B)])
    neg = c["pos"][others].contiguous()
    g2, rw2 = t.zeros(U + I, d, device=DEV), t.zeros(U + I, device=DEV)
    # lambda = 0 there and the L2 term apart: the M-negative loss also counts the rows of its negatives
    loss2 = ops.rank_loss_fwd_bwd(c["users"].to(DEV), c["pos"].to(DEV), neg.to(DEV), c["final"].to(DEV), c["e0"].to(DEV), U,
                                  0.0, objective="softmax", g_final=g2, reg_w=rw2, logq=None if logq is None else logq.to(DEV))
    l2 = lam * (c["e0"][c["users"]].double().pow(2).sum() + c["e0"][U + c["pos"]].double().pow(2).sum())
    print(f"logq={with_logq}: in-batch {float(loss):.9f}, M = 16 kernel + L2 {float(loss2) + float(l2):.9f}, "
          f"max |dg| {float((gf - g2).abs().max()):.3e}")
    assert _loss_close(loss, float(loss2) + float(l2))
    assert t.allclose(gf, g2, atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 5: refusals
def test_refusals():
    ops = _ops()
    from laplace_amd._lib import MiError
    u, p = t.zeros(64, dtype=t.int64, device=DEV), t.zeros(64, dtype=t.int64, device=DEV)
    for d in (260, 30):
        with pytest.raises((MiError, ValueError)):
            ops.inbatch_softmax_fwd_bwd(u, p, t.zeros(9, d, device=DEV), t.zeros(9, d, device=DEV), 4, 1e-6, group=32)
    with pytest.raises((MiError, ValueError)):
        ops.inbatch_softmax_fwd_bwd(u, p, t.zeros(9, 32, device=DEV), t.zeros(9, 32, device=DEV), 4, 1e-6, group=48)
    # the library's own answers, past the Python checks
    from laplace_amd import _lib
    L = _lib.lib()
    x, out = t.zeros(9, 260, device=DEV), t.zeros(1, device=DEV)
    ws = t.zeros(L.mi_inbatch_softmax_workspace_bytes(64, 32, 32), dtype=t.uint8, device=DEV)

    def raw(d, group):
        return L.mi_inbatch_softmax_fwd_bwd_f32(64, group, d, 4, u.data_ptr(), p.data_ptr(), x.data_ptr(), 260, x.data_ptr(),
                                                260, 1e-6, 1.0, 1.0, out.data_ptr(), None, 0, None, None, None, ws.data_ptr(),
                                                ws.numel(), None)
    assert raw(260, 32) == _lib.MI_ERR_UNSUPPORTED and raw(30, 32) == _lib.MI_ERR_UNSUPPORTED
    assert raw(32, 48) == _lib.MI_ERR_BAD_ARG and raw(32, 32) == 0


# ---------------------------------------------------------------------------- 6: autograd function
def test_autograd_function_with_ids_and_logq():
    from laplace_amd.utils.metrics_lightgcn import in_batch_softmax_loss
    c = T.cases()[3]                                     # 5 users, 6 items: every id repeats
    U, lam = c["U"], 1e-2
    users, pos = c["users"], c["pos"]
    want, g_fin, g_e0 = T.reference(3, lam, True)
    f = c["final"].to(DEV).requires_grad_(True)
    e = c["e0"].to(DEV).requires_grad_(True)
    ud, pd = users.to(DEV), pos.to(DEV)
    loss = in_batch_softmax_loss(f[ud], e[ud], f[U + pd], e[U + pd], lam, user_ids=ud, item_ids=pd,
                                 logq=c["logq"].to(DEV)[pd], group=c["G"])
    (2.0 * loss).backward()
    assert _loss_close(loss.detach(), want)
    assert t.allclose(f.grad.cpu().double(), 2.0 * g_fin, atol=2e-6, rtol=1e-4)
    assert t.allclose(e.grad.cpu().double(), 2.0 * g_e0, atol=2e-6, rtol=1e-4)
    # without ids nothing is masked: the twin on one row per slot
    B = c["B"]
    a = t.arange(B)
    tab = t.cat([c["final"][users], c["final"][U + pos]])
    tab0 = t.cat([c["e0"][users], c["e0"][U + pos]])
    want2 = T.twin(tab, tab0, B, a, a, c["G"], lam, None, t.float64)[0]
    loss2 = in_batch_softmax_loss(f[ud], e[ud], f[U + pd], e[U + pd], lam, group=c["G"])
    assert _loss_close(loss2.detach(), want2) and abs(float(loss2) - float(loss)) > 1e-3


# ---------------------------------------------------------------------------- 7: trainer
def _model_and_graph(U, I, n_edges, D, K, seed):
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    g = t.Generator().manual_seed(seed)
    ei = t.stack([t.randint(0, U, (n_edges,), generator=g), t.randint(0, I, (n_edges,), generator=g)])
    t.manual_seed(seed)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K)
    inter = Interactions(ei, U, I)
    return model, inter, inter.adjacency("bipartite"), ei


GRAPH = dict(U=400, I=300, n_edges=6000, D=64, K=3, seed=23)
B_TRAIN, G_TRAIN, LAM_TRAIN, STEPS = 160, 64, 1e-5, 6


def _trainer(**kw):
    from laplace_amd.trainer import LightGCNTrainer
    model, inter, adj, _ = _model_and_graph(**GRAPH)
    model.to(DEV)
    kw.setdefault("negatives", "in_batch")
    if kw["negatives"] == "in_batch":
        kw.setdefault("in_batch_group", G_TRAIN)
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
    seed 5, and a negatives="uniform" run made BEFORE any in-batch trainer exists."""
    uniform_before = _run(negatives="uniform", n_neg=1)
    model, inter, adj, _ = _model_and_graph(**GRAPH)
    U, I, K = GRAPH["U"], GRAPH["I"], GRAPH["K"]
    uw = t.nn.Parameter(model.users_emb.weight.detach().clone())
    iw = t.nn.Parameter(model.items_emb.weight.detach().clone())
    opt = t.optim.Adam([uw, iw], lr=1e-3)
    row, col, _ = adj.coo()
    degree = t.bincount(inter.edge_index[1].cpu(), minlength=I)
    from laplace_amd import ops
    logq = ops.negative_table(degree, 1.0, device="cpu").logq
    batches, losses = [], []
    for users, pos, _neg in uniform_before[1]:
        ui, pi = users.cpu(), pos.cpu()
        uf, u0, itf, it0 = R.lightgcn_forward(uw, iw, row, col, K)
        want = T.twin_loss(t.cat([uf, itf]), t.cat([u0, it0]), U, ui, pi, G_TRAIN, LAM_TRAIN, logq)
        opt.zero_grad()
        want.backward()
        opt.step()
        batches.append((users, pos))
        losses.append(float(want))
    return dict(batches=batches, losses=losses, uw=uw.detach(), iw=iw.detach(), uniform_before=uniform_before, logq=logq)


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("sparse_batch", [False, True])
def test_trainer_six_steps_match_autograd_loop(autograd_run, sparse_batch, reorder):
    ref = autograd_run
    losses, _, table, tr = _run(batches=ref["batches"], sparse_batch=sparse_batch, reorder=reorder)
    assert tr.logq_correction and tr.in_batch and tr.in_batch_group == G_TRAIN and (tr.order is not None) == reorder
    U = GRAPH["U"]
    du = float((table[:U].cpu() - ref["uw"]).abs().max())
    di = float((table[U:].cpu() - ref["iw"]).abs().max())
    print(f"sparse_batch={sparse_batch} reorder={reorder}: max |dloss| "
          f"{max(abs(a - b) for a, b in zip(losses, ref['losses'])):.3e}, max |dtable| {max(du, di):.3e}")
    for a, b in zip(losses, ref["losses"]):
        assert _loss_close(a, b)
    assert du <= 1e-4 and di <= 1e-4
    # the logq table is the degree proposal, in the id space the kernels train in
    lq = tr.logq.cpu()
    assert t.equal(lq[tr.order.item_new_of_old.cpu()] if reorder else lq, ref["logq"])
    # bitwise reproducible, fuse_adam on or off, and a 3-tuple's third entry is ignored
    again = _run(batches=ref["batches"], sparse_batch=sparse_batch, reorder=reorder)
    assert again[0] == losses and t.equal(again[2], table)
    junk = [(u, p, t.zeros_like(p)) for u, p in ref["batches"]]
    unfused = _run(batches=junk, sparse_batch=sparse_batch, reorder=reorder, fuse_adam=False)
    assert unfused[0] == losses and t.equal(unfused[2], table)


def test_trainer_draws_the_uniform_edge_stream_and_leaks_no_state(autograd_run):
    ref = autograd_run
    before = ref["uniform_before"]
    own = _run()                                          # the in-batch trainer's own batches
    for (u, p, _), (u2, p2, _) in zip(own[1], before[1]):
        assert t.equal(u, u2) and t.equal(p, p2)
    given = _run(batches=ref["batches"])
    assert own[0] == given[0] and t.equal(own[2], given[2])
    uncorrected = _run(batches=ref["batches"], logq_correction=False)
    assert uncorrected[3].logq is None and max(abs(a - b) for a, b in zip(uncorrected[0], given[0])) > 1e-3
    after = _run(negatives="uniform", n_neg=1)            # a uniform trainer after the in-batch ones: as before them
    assert after[0] == before[0] and t.equal(after[2], before[2])
    assert after[3].logq is None and not after[3].in_batch


def test_pipeline_passes_in_batch_negatives_through(tmp_path):
    """run_pipeline_lightgcn.train under compat="reference", whose negative range and sampler quirk in-batch negatives leave
    out: the run ends with finite statistics, and another group size gives another training loss."""
    import math
    from dataclasses import replace
    from laplace_amd.config import lightgcn_config
    from laplace_amd.run_pipeline_lightgcn import train
    from test_gpu_acceptance import _tastes_graph
    cfg = replace(lightgcn_config, epochs=30, k=12, hidden_layer_size=32, learning_rate=1e-3, save_model=False, batch_size=128,
                  num_iterations=2, eval_every=100, lr_decay_every=100, Lambda=1e-6, show_graph=False, num_recommendations=64)
    ei = t.from_numpy(_tastes_graph(300, 200, 1000, seed=42).T.copy())
    out = {}
    for group in (32, 128):
        t.manual_seed(42)
        stats = train(cfg, edge_index=ei, num_users=300, num_articles=200, compat="reference", device=DEV, seed=42,
                      verbose=False, save_dir=str(tmp_path / str(group)), objective="softmax", predictor="propagated",
                      negatives="in_batch", in_batch_group=group)
        for v in (stats.loss, stats.recall_val, stats.recall_test, stats.precision_val, stats.precision_test):
            assert math.isfinite(v)
        out[group] = stats.loss
    assert out[32] != out[128]
    with pytest.raises(ValueError):
        train(cfg, edge_index=ei, num_users=300, num_articles=200, device=DEV, verbose=False, objective="softmax",
              negatives="in_batch", in_batch_group=48)


# ---------------------------------------------------------------------------- 8: quality floor
def test_in_batch_negatives_beat_the_popularity_predictor():
    """The `worth` recipe of tools/bench_inbatch.py (that of profiles/neg_sampling.md section 4: C1-scale planted graph, spec
    seed 5, D 64, K 2, batch 1024, lr 1e-2, lambda 1e-6, 200 steps, bench.map_at_12) at trainer seed 7, G = 256, corrected:
    the propagated MAP@12 must reach the popularity predictor's, scored in the same call."""
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
                         objective="softmax", negatives="in_batch", in_batch_group=256)
    got = bench.map_at_12(model, tr, inter, held, 200)
    print("in-batch G=256 corrected: propagated MAP@12", got["propagated_embeddings_map_at_12"], "layer-0", got["value"],
          "popularity", got["popularity_predictor_map_at_12"], "loss", float(tr.loss))
    assert got["propagated_embeddings_map_at_12"] >= got["popularity_predictor_map_at_12"]
