"""GPU: the noise-view contrastive term — mi_perturb_rows_f32 against the numpy mirror of the noise, mi_contrastive_fwd_bwd_f32
against its float64 twin (tests/contrastive_emulation.py), their refusals, the trainer with cl_weight > 0 against an fp32
autograd loop over the twin with the mirror's noise injected, and the pipeline's keywords.

Tolerances.  Perturb kernel: derived in contrastive_emulation.perturb_bound, eps * (d + 8) * 2^-24 + 2^-23 * |Y| per element; the
S form adds the rounding of the sum and of the product with the scale, 2^-24 * (|addend + X| * scale + |S|).  Contrast: the
in-batch softmax's (tests/test_gpu_inbatch_softmax.py): loss 1e-6 * max(1, |loss|), gradients atol 1e-6 / rtol 1e-4.  The
gradient tables are pre-filled, and the call adds: against (after - before) the tolerance gains the rounding of that one
addition, 2^-24 * |after| (the pre-fill is at most 1/8 in magnitude: about 1e-8).  Trainer: that test's, losses 1e-6 *
max(1, |loss|) and tables 1e-4 after six steps.

sign() is discontinuous, so the trainer can only be compared with a twin whose propagated values have the same signs.  The
twin asserts, on its own, that no propagated element has 0 < |y| < 1e-6 in any layer of any step.  With the model's own
N(0, 0.1) table no choice of seed gives that: the 700 x 64 elements of up to 3 layers over 6 steps are some 800 000 draws
with a density of about 18 per unit around zero, some 30 of them below 1e-6 in a run (smallest |y| of the three seeds tried
on the CPU: 1.2e-8 to 1.9e-7).  The test's table is therefore the model's with the sign of column c set to (-1)^c and 0.05
added to every magnitude: A has no negative entry, so every propagated element of a node with an edge keeps its column's sign
at a magnitude the six steps (lr 1e-3: at most 6e-3 per entry) cannot bring near zero, and both signs are exercised."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contrastive_emulation as E  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 0.2


def _ops():
    from laplace_amd import ops
    return ops


def _loss_close(got, want):
    return abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


# ---------------------------------------------------------------------------- 1: the perturb kernel vs the mirror
def _layer(rows, d):
    """Y [rows, d] as columns [0, d) of a [rows, d + 4] buffer (leading dimension > d), with an all-zero row and a row holding
    -0.0 where there are rows enough (one row: a -0.0 element)."""
    g = t.Generator().manual_seed(100 * rows + d)
    wide = t.randn(rows, d + 4, generator=g)
    if rows >= 3:
        wide[rows // 2, :d] = 0.0
        wide[rows - 1, : d // 2] = -0.0
    else:
        wide[0, 0] = -0.0
    return wide


@pytest.mark.parametrize("d", [4, 36, 128, 256])
@pytest.mark.parametrize("rows", [1, 63, 70, 257])
def test_perturb_rows_matches_the_mirror_in_every_form(rows, d):
    ops = _ops()
    wide = _layer(rows, d)
    y = wide[:, :d].numpy().copy()
    kw = dict(eps=EPS, layer=2, seed=9, step=4)
    want = E.perturb(y, EPS, 2, 9, 4)
    bound = E.perturb_bound(y, EPS)

    def run(x_wide=None, **more):
        buf = (wide if x_wide is None else x_wide).to(DEV)
        ops.perturb_rows(buf[:, :d], **kw, **more)
        return buf.cpu()
    got = run()
    err = np.abs(got[:, :d].double().numpy() - want)
    print(f"rows={rows} d={d}: max err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    assert t.equal(got[:, d:], wide[:, d:])                               # beyond d: not touched
    if rows >= 3:
        assert float(got[rows // 2, :d].abs().max()) == 0.0               # the all-zero row stays zero
        assert float(got[rows - 1, : d // 2].abs().max()) == 0.0          # -0.0 has no sign to follow
    assert t.equal(run(), got)                                            # two calls, equal bits
    assert t.equal(run(row_ids=t.arange(rows, device=DEV)), got)          # the identity, or no row_ids
    for other in (dict(step=5), dict(layer=1), dict(seed=10)):
        buf = wide.to(DEV)
        ops.perturb_rows(buf[:, :d], **{**kw, **other})
        assert not t.equal(buf.cpu(), got), other
    # a permuted row_ids: the noise follows the id
    perm = t.randperm(rows, generator=t.Generator().manual_seed(rows))
    assert t.equal(run(x_wide=wide[perm].contiguous(), row_ids=perm.to(DEV))[:, :d], got[perm][:, :d])
    # S = (addend + X) * scale in the same pass; S may be the addend itself
    g = t.Generator().manual_seed(d)
    addend = t.randn(rows, d + 8, generator=g)
    for scale in (1.0, 1.0 / 3.0):
        x_dev, a_dev, s_dev = wide.to(DEV), addend.to(DEV), t.full((rows, d + 4), 7.0, device=DEV)
        ops.perturb_rows(x_dev[:, :d], **kw, addend=a_dev[:, :d], S=s_dev[:, :d], scale=scale)
        assert t.equal(x_dev.cpu(), got) and t.equal(s_dev[:, d:].cpu(), t.full((rows, 4), 7.0))
        total = addend[:, :d].double().numpy() + want
        s_want = total * float(np.float32(scale))                         # the scale arrives as an fp32 number
        s_bound = (bound + 2.0 ** -24 * np.abs(total)) * scale + 2.0 ** -24 * np.abs(s_want)
        assert np.all(np.abs(s_dev[:, :d].cpu().double().numpy() - s_want) <= s_bound)
        x2, alias = wide.to(DEV), addend.to(DEV)
        ops.perturb_rows(x2[:, :d], **kw, addend=alias[:, :d], S=alias[:, :d], scale=scale)
        assert t.equal(alias[:, :d], s_dev[:, :d]) and t.equal(alias[:, d:].cpu(), addend[:, d:])
    x3, s3 = wide.to(DEV), t.empty(rows, d, device=DEV)
    ops.perturb_rows(x3[:, :d], **kw, S=s3, scale=0.5)                    # no addend: S = X * scale
    assert t.equal(s3.cpu(), got[:, :d] * 0.5)


@pytest.mark.parametrize("d", [4, 36, 256])
def test_first_rows_of_a_larger_call_equal_a_smaller_call(d):
    ops = _ops()
    y = t.randn(70, d, generator=t.Generator().manual_seed(d))
    big, small = y.to(DEV), y[:10].to(DEV)
    ops.perturb_rows(big, eps=EPS, layer=1, seed=3, step=0)
    ops.perturb_rows(small, eps=EPS, layer=1, seed=3, step=0)
    assert t.equal(big[:10], small) and not t.equal(big.cpu(), y)


# ---------------------------------------------------------------------------- 2: the contrast vs the float64 twin
def _prefill(shape, seed):
    """Non-zero multiples of 2^-10 in [-1/8, 1/8]."""
    k = t.randint(1, 129, shape, generator=t.Generator().manual_seed(seed))
    s = t.randint(0, 2, shape, generator=t.Generator().manual_seed(seed + 1)) * 2 - 1
    return (k * s).float() / 1024.0


def _device_contrast(c, g_scale_a=1.0, g_scale_b=1.0, want_grad=True):
    ops = _ops()
    a, b, ids = c["a"].to(DEV), c["b"].to(DEV), c["ids"].to(DEV)
    if not want_grad:
        return ops.contrastive_fwd_bwd(ids, a, b, tau=c["tau"], group=c["G"]), None, None
    g_a, g_b = _prefill(a.shape, 1).to(DEV), _prefill(b.shape, 3).to(DEV)
    loss = ops.contrastive_fwd_bwd(ids, a, b, tau=c["tau"], group=c["G"], g_a=g_a, g_b=g_b, g_scale_a=g_scale_a,
                                   g_scale_b=g_scale_b)
    return loss, g_a.cpu(), g_b.cpu()


def _added_close(after, before, want):
    diff = after.double() - before.double()
    tol = 1e-6 + 1e-4 * want.abs() + 2.0 ** -24 * after.double().abs()
    return bool(((diff - want).abs() <= tol).all())


@pytest.mark.parametrize("duplicated", [False, True])
@pytest.mark.parametrize("d", E.WIDTHS)
@pytest.mark.parametrize("G", E.GROUPS)
@pytest.mark.parametrize("B", E.BATCHES)
def test_contrast_matches_float64_twin_and_adds_to_its_gradient_tables(B, G, d, duplicated):
    c = E.case(B, G, d, duplicated)
    want, wa, wb = E.reference(B, G, d, duplicated)
    loss, g_a, g_b = _device_contrast(c)
    pa, pb = _prefill(c["a"].shape, 1), _prefill(c["b"].shape, 3)
    print(f"B={B} G={G} d={d} dup={duplicated}: loss {float(loss):.9f} want {float(want):.9f} |dloss| "
          f"{abs(float(loss) - float(want)):.3e} max |dg_a| {float((g_a.double() - pa.double() - wa).abs().max()):.3e} "
          f"max |dg_b| {float((g_b.double() - pb.double() - wb).abs().max()):.3e}")
    assert _loss_close(loss, want)
    assert _added_close(g_a, pa, wa) and _added_close(g_b, pb, wb)
    untouched = t.ones(E.N_ROWS, dtype=t.bool)
    untouched[c["ids"]] = False
    assert t.equal(g_a[untouched], pa[untouched]) and t.equal(g_b[untouched], pb[untouched])
    if B > 1 and not (duplicated and len(set(c["ids"][: G].tolist())) == 1):
        assert float((g_a - pa).abs().max()) > 0.0
    # a second call and the loss-only form: equal bits
    again = _device_contrast(c)
    assert t.equal(again[0], loss) and t.equal(again[1], g_a) and t.equal(again[2], g_b)
    assert t.equal(_device_contrast(c, want_grad=False)[0], loss)


@pytest.mark.parametrize("B,G,d,duplicated", [(33, 32, 4, True), (96, 32, 64, False), (160, 64, 256, True)])
def test_contrast_gradient_scales(B, G, d, duplicated):
    c = E.case(B, G, d, duplicated)
    want, wa, wb = E.reference(B, G, d, duplicated)
    loss, g_a, g_b = _device_contrast(c, g_scale_a=0.25, g_scale_b=2.0)
    assert _loss_close(loss, want)                       # the scales do not touch the loss value
    assert _added_close(g_a, _prefill(c["a"].shape, 1), 0.25 * wa) and _added_close(g_b, _prefill(c["b"].shape, 3), 2.0 * wb)


def _loss_bits_tool():
    """tools/record_loss_bits.py: the cases of tests/golden/tile_loss_bits.json and the function that records one."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_loss_bits
    return record_loss_bits


@pytest.mark.parametrize("B", E.BATCHES)
def test_every_shape_gives_its_recorded_bits(B):
    """Loss, g_a, g_b (zero on entry, g_scale_a = 1/3, g_scale_b = 1) and the loss-only form's loss of every group, width and
    kind of ids at batch B, against the bits recorded at the commit tests/golden/tile_loss_bits.json names.  The cases and
    the recording are the tool's: neither side changes alone."""
    tool = _loss_bits_tool()
    with open(os.path.join(ROOT, "tests", "golden", "tile_loss_bits.json")) as f:
        rec = json.load(f)["contrastive"]
    assert len(rec) == len(E.BATCHES) * len(E.GROUPS) * len(E.WIDTHS) * 2
    cases = tool.contrastive_cases(B)
    assert len(cases) == len(E.GROUPS) * len(E.WIDTHS) * 2
    for c in cases:
        assert tool.contrastive_record(c) == rec[c["key"]], c["key"]


def test_autograd_function_over_gathered_blocks():
    from laplace_amd.utils.metrics_lightgcn import contrastive_loss
    B, G, d = 96, 32, 64
    c = E.case(B, G, d, True)
    want, wa, wb = E.reference(B, G, d, True)
    a = c["a"].to(DEV).requires_grad_(True)
    b = c["b"].to(DEV).requires_grad_(True)
    ids = c["ids"].to(DEV)
    loss = contrastive_loss(a[ids], b[ids], ids, c["tau"], G)
    (2.0 * loss).backward()
    assert _loss_close(loss.detach(), want)
    assert t.allclose(a.grad.cpu().double(), 2.0 * wa, atol=2e-6, rtol=1e-4)
    assert t.allclose(b.grad.cpu().double(), 2.0 * wb, atol=2e-6, rtol=1e-4)
    # without ids nothing is masked: the twin on one row per slot
    slots = t.arange(B)
    want2 = E.contrast_twin(c["a"][c["ids"]], c["b"][c["ids"]], slots, c["tau"], G)[0]
    loss2 = contrastive_loss(a[ids], b[ids], None, c["tau"], G)
    assert _loss_close(loss2.detach(), want2) and abs(float(loss2) - float(loss)) > 1e-3


# ---------------------------------------------------------------------------- 3: refusals
def test_refusals_fire_before_any_launch():
    ops = _ops()
    from laplace_amd import _lib
    from laplace_amd._lib import MiError
    L = _lib.lib()
    ids = t.zeros(64, dtype=t.int64, device=DEV)
    x = t.ones(9, 32, device=DEV)
    for d in (260, 30):
        with pytest.raises(ValueError):
            ops.contrastive_fwd_bwd(ids, t.zeros(9, d, device=DEV), t.zeros(9, d, device=DEV), tau=0.15, group=32)
        with pytest.raises(ValueError):
            ops.perturb_rows(t.zeros(9, d, device=DEV), eps=EPS, layer=1, seed=0, step=0)
    for bad in (dict(group=48), dict(tau=0.0), dict(g_a=t.zeros(9, 32, device=DEV))):
        with pytest.raises(ValueError):
            ops.contrastive_fwd_bwd(ids, x, x, **{**dict(tau=0.15, group=32), **bad})
    with pytest.raises(TypeError):
        ops.contrastive_fwd_bwd(ids.int(), x, x, tau=0.15, group=32)
    for bad in (dict(eps=-0.1), dict(layer=-1), dict(addend=x.clone()), dict(row_ids=t.arange(8, device=DEV)),
                dict(S=t.zeros(9, 36, device=DEV))):
        with pytest.raises(ValueError):
            ops.perturb_rows(x, **{**dict(eps=EPS, layer=1, seed=0, step=0), **bad})
    with pytest.raises(MiError):                         # S is x itself: the library's own answer
        ops.perturb_rows(x, eps=EPS, layer=1, seed=0, step=0, S=x)
    assert t.equal(x.cpu(), t.ones(9, 32))               # nothing ran
    # the library's own answers, past the Python checks
    wide, out = t.zeros(9, 260, device=DEV), t.zeros(1, device=DEV)
    ws = t.zeros(L.mi_contrastive_workspace_bytes(64, 32, 32), dtype=t.uint8, device=DEV)

    def raw(d, group, inv_tau=6.0, g_a=None):
        return L.mi_contrastive_fwd_bwd_f32(64, group, d, ids.data_ptr(), wide.data_ptr(), 260, wide.data_ptr(), 260, inv_tau,
                                            out.data_ptr(), g_a, 260, 1.0, None, 260, 1.0, ws.data_ptr(), ws.numel(), None)
    assert raw(260, 32) == _lib.MI_ERR_UNSUPPORTED and raw(30, 32) == _lib.MI_ERR_UNSUPPORTED
    assert raw(32, 32, g_a=wide.data_ptr()) == _lib.MI_ERR_UNSUPPORTED
    assert raw(32, 48) == _lib.MI_ERR_BAD_ARG and raw(32, 32, inv_tau=0.0) == _lib.MI_ERR_BAD_ARG and raw(32, 32) == 0

    def raw_perturb(d, eps=EPS, ldx=260):
        return L.mi_perturb_rows_f32(9, d, wide.data_ptr(), ldx, None, eps, 1, 0, 0, None, 0, None, 0, 1.0, None)
    assert raw_perturb(260) == _lib.MI_ERR_UNSUPPORTED and raw_perturb(30) == _lib.MI_ERR_UNSUPPORTED
    assert raw_perturb(32, eps=-1.0) == _lib.MI_ERR_BAD_ARG and raw_perturb(32, ldx=30) == _lib.MI_ERR_BAD_ARG
    assert float(wide.abs().max()) == 0.0 and raw_perturb(32) == 0


# ---------------------------------------------------------------------------- 4: trainer
GRAPH = dict(U=400, I=300, n_edges=6000, D=64, seed=23)
B_TRAIN, G_TRAIN, LAM_TRAIN, LR, STEPS, SEED = 160, 64, 1e-5, 1e-3, 6, 5
CL = dict(cl_weight=0.2, cl_eps=EPS, cl_tau=0.15, cl_group=G_TRAIN)
OBJECTIVES = {"reference": dict(objective="reference"), "softmax4": dict(objective="softmax", n_neg=4)}


def _model_and_graph(K):
    """The 400 x 300 graph of 6 000 edges at D = 64 of tests/test_gpu_inbatch_softmax.py; the table's column c carries the sign
    (-1)^c at magnitudes >= 0.05 (the module's header says why)."""
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    U, I, n_edges, D, seed = (GRAPH[k] for k in ("U", "I", "n_edges", "D", "seed"))
    g = t.Generator().manual_seed(seed)
    ei = t.stack([t.randint(0, U, (n_edges,), generator=g), t.randint(0, I, (n_edges,), generator=g)])
    t.manual_seed(seed)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K)
    with t.no_grad():
        tab = model.table()
        sign = 1.0 - 2.0 * (t.arange(D) % 2).float()
        tab.copy_((tab.abs() + 0.05) * sign)
    inter = Interactions(ei, U, I)
    return model, inter, inter.adjacency("bipartite")


def _trainer(K, **kw):
    from laplace_amd.trainer import LightGCNTrainer
    model, inter, adj = _model_and_graph(K)
    model.to(DEV)
    kw.setdefault("sparse_batch", False)
    return model, LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), lr=LR, Lambda=LAM_TRAIN, batch_size=B_TRAIN, seed=SEED, **kw)


def _run(K, batches=None, **kw):
    model, tr = _trainer(K, **kw)
    losses, used = [], []
    for i in range(STEPS):
        batch = batches[i] if batches is not None else tuple(x.clone() for x in tr.sample())
        used.append(batch)
        losses.append(float(tr.step(batch)))
    tr.finish()
    return losses, used, tr.table.clone(), tr


@pytest.fixture(scope="module")
def twin_runs():
    """(K, cl_layer, objective) -> the batches the sampler draws at SEED and six steps of the fp32 autograd loop over the twin
    on them; computed once per key, shared by the trainer tests."""
    cache = {}

    def get(K, layer, objective):
        key = (K, layer, objective)
        if key not in cache:
            _, tr = _trainer(K, **OBJECTIVES[objective])         # cl_weight = 0: only its sampler is used
            batches = []
            for _ in range(STEPS):
                batches.append(tuple(x.clone() for x in tr.sample()))
                tr.step_count += 1
            model, inter, adj = _model_and_graph(K)
            row, col, _ = adj.coo()
            losses, uw, iw, smallest = E.train_twin(
                model.users_emb.weight, model.items_emb.weight, row, col, K, [tuple(x.cpu() for x in b) for b in batches],
                lam=LAM_TRAIN, lr=LR, objective=OBJECTIVES[objective]["objective"], cl_weight=CL["cl_weight"], cl_eps=EPS,
                cl_tau=CL["cl_tau"], cl_layer=layer, cl_group=G_TRAIN, seed=SEED)
            print(f"twin K={K} layer={layer} {objective}: smallest non-zero |y| {smallest:.3e}")
            assert smallest >= 1e-6                              # on the twin alone: no sign can differ on the device
            cache[key] = dict(batches=batches, losses=losses, uw=uw, iw=iw)
        return cache[key]
    return get


@pytest.mark.parametrize("objective", sorted(OBJECTIVES))
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("K,layer", [(3, 1), (3, 3), (1, 1)])
def test_trainer_six_steps_match_autograd_loop(twin_runs, K, layer, reorder, objective):
    ref = twin_runs(K, layer, objective)
    kw = dict(reorder=reorder, cl_layer=layer, **CL, **OBJECTIVES[objective])
    losses, _, table, tr = _run(K, batches=ref["batches"], **kw)
    assert tr.cl_weight == CL["cl_weight"] and (tr.order is not None) == reorder and tr.step_count == STEPS
    U = GRAPH["U"]
    du = float((table[:U].cpu() - ref["uw"]).abs().max())
    di = float((table[U:].cpu() - ref["iw"]).abs().max())
    print(f"K={K} layer={layer} reorder={reorder} {objective}: max |dloss| "
          f"{max(abs(a - b) for a, b in zip(losses, ref['losses'])):.3e}, max |dtable| {max(du, di):.3e}")
    for a, b in zip(losses, ref["losses"]):
        assert _loss_close(a, b)
    assert du <= 1e-4 and di <= 1e-4
    assert float(tr.g_cl.abs().max()) == 0.0                     # the layer gradient's rows are zero again
    # bitwise reproducible, fuse_adam on or off
    again = _run(K, batches=ref["batches"], **kw)
    assert again[0] == losses and t.equal(again[2], table)
    unfused = _run(K, batches=ref["batches"], fuse_adam=False, **kw)
    assert unfused[0] == losses and t.equal(unfused[2], table)
    # the term is there: without it the run differs
    plain = _run(K, batches=ref["batches"], reorder=reorder, **OBJECTIVES[objective])
    assert max(abs(a - b) for a, b in zip(plain[0], losses)) > 1e-3


@pytest.mark.parametrize("sparse_batch", [False, True])
def test_zero_weight_is_the_trainer_without_the_keywords(sparse_batch):
    base = _run(3, sparse_batch=sparse_batch)
    zero = _run(3, sparse_batch=sparse_batch, cl_weight=0.0, cl_eps=0.3, cl_tau=0.5, cl_layer=2, cl_group=32)
    assert zero[0] == base[0] and t.equal(zero[2], base[2])
    assert not hasattr(zero[3], "x_cl")


@pytest.mark.parametrize("reorder", [False, True])
def test_forward_of_a_contrastive_trainer_is_the_unperturbed_propagate(reorder):
    _, tr = _trainer(3, reorder=reorder, cl_layer=1, **CL)
    _, plain = _trainer(3, reorder=reorder)
    assert t.equal(tr.forward(), plain.forward())
    tr.step()
    plain.table.copy_(tr.table)
    assert t.equal(tr.forward(), plain.forward())


def test_trainer_combines_with_in_batch_negatives_and_the_full_softmax():
    for kw in (dict(objective="softmax", negatives="in_batch", in_batch_group=64), dict(objective="softmax", full_softmax=True)):
        a = _run(2, cl_layer=2, **CL, **kw)
        b = _run(2, cl_layer=2, **CL, **kw)
        plain = _run(2, **kw)
        assert all(math.isfinite(x) for x in a[0]) and a[0] == b[0] and t.equal(a[2], b[2])
        assert max(abs(x - y) for x, y in zip(a[0], plain[0])) > 1e-3


# ---------------------------------------------------------------------------- 5: pipeline
def test_pipeline_passes_the_contrastive_keywords_through(tmp_path):
    from dataclasses import replace
    from laplace_amd.config import lightgcn_config
    from laplace_amd.run_pipeline_lightgcn import train
    from test_gpu_acceptance import _tastes_graph
    cfg = replace(lightgcn_config, epochs=30, k=12, hidden_layer_size=32, learning_rate=1e-3, save_model=False, batch_size=128,
                  num_iterations=2, eval_every=100, lr_decay_every=100, Lambda=1e-6, show_graph=False, num_recommendations=64)
    ei = t.from_numpy(_tastes_graph(300, 200, 1000, seed=42).T.copy())
    out = {}
    for name, kw in (("off", dict()), ("on", dict(cl_weight=0.2, cl_group=64)), ("layer2", dict(cl_weight=0.2, cl_group=64, cl_layer=2)),
                     ("tau", dict(cl_weight=0.2, cl_group=64, cl_tau=0.5)), ("eps", dict(cl_weight=0.2, cl_group=64, cl_eps=0.05))):
        t.manual_seed(42)
        stats = train(cfg, edge_index=ei, num_users=300, num_articles=200, compat="reference", device=DEV, seed=42,
                      verbose=False, save_dir=str(tmp_path / name), objective="softmax", n_neg=4, predictor="propagated", **kw)
        for v in (stats.loss, stats.recall_val, stats.recall_test, stats.precision_val, stats.precision_test):
            assert math.isfinite(v)
        out[name] = stats.loss
    assert len(set(out.values())) == len(out)            # every keyword reaches the trainer
    with pytest.raises(ValueError):
        train(cfg, edge_index=ei, num_users=300, num_articles=200, device=DEV, verbose=False, cl_weight=0.2, cl_layer=3)
