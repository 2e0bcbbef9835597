"""GPU: the sparse trainer — torch.optim.SparseAdam's update on the rows a batch references (mi_lazy_adam_rows_f32,
mi_pinsage_project_bwd_lazy_f32, mi_pinsage_text_bwd_lazy_f32) against tests/lazy_adam_emulation.py over the summed rows of
tests/segsum_emulation.py, bit for bit; PinSAGEModel(sparse_tables=True) on NativePinSAGEStep against the autograd path with
torch.optim.Adam + torch.optim.SparseAdam; checkpoints across the two; state that outlives a call."""
import copy
import ctypes

import numpy as np
import pytest
import torch as t

import lazy_adam_emulation as LE
import segsum_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
HYPER = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8)


def _lazy(step, **kw):
    from laplace_amd import _lib
    h = {**HYPER, **kw}
    z = _lib.LazyAdam()
    z.lr, z.beta1, z.beta2, z.eps, z.step = h["lr"], h["beta1"], h["beta2"], h["eps"], step
    return z


def _bits(x):
    return (x.detach().cpu().numpy() if isinstance(x, t.Tensor) else x).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


# ---- 1. the row update -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 20, 128, 512])
def test_lazy_adam_rows_bits_are_the_emulation(width):
    """n in {0, 1, 63, 300} distinct rows of 400 (the last row never among them), three consecutive steps on the same tables,
    gradient rows with a leading dimension wider than the row; from the second step on the first referenced row has a zero
    gradient over live moments and must still move."""
    from laplace_amd import _lib
    L = _lib.lib()
    R = 400
    rng = np.random.default_rng(width)
    for n in (0, 1, 63, 300):
        p = rng.standard_normal((R, width)).astype(np.float32)
        m, v = np.zeros_like(p), np.zeros_like(p)
        dp, dm, dv = (t.from_numpy(x.copy()).to(DEV) for x in (p, m, v))
        first = int(rng.integers(0, R - 1))
        for step in (1, 2, 3):
            rows = rng.choice(R - 1, n, replace=False)
            if n:
                rows[rows == first] = rows[0]
                rows[0] = first                                           # referenced on every step
            ldg = width + 4
            g = (rng.standard_normal((n, ldg)) * 10.0 ** rng.uniform(-4, 1)).astype(np.float32)
            if n and step > 1:
                g[0] = 0.0
            snap = (p.copy(), m.copy(), v.copy())
            LE.update_rows(p, m, v, rows, g[:, :width], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], step)
            ids, dg = t.from_numpy(rows.astype(np.int64)).to(DEV), t.from_numpy(g).to(DEV)
            _lib.check(L.mi_lazy_adam_rows_f32(R, width, dp.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, ids.data_ptr() if n else None,
                                               dg.data_ptr() if n else None, ldg, ctypes.byref(_lazy(step)), _lib.current_stream()),
                       "mi_lazy_adam_rows_f32")
            for name, got, want, was in (("p", dp, p, snap[0]), ("m", dm, m, snap[1]), ("v", dv, v, snap[2])):
                assert _same_bits(got, want), (n, step, name)             # referenced rows: the emulation; the others: unchanged
                rest = np.setdiff1d(np.arange(R), rows)
                assert R - 1 in rest and _same_bits(got.cpu().numpy()[rest], was[rest]), (n, step, name)
            if n and step > 1:
                for got, was in ((dp, snap[0]), (dm, snap[1]), (dv, snap[2])):
                    assert not np.array_equal(got.cpu().numpy()[first], was[first]), (n, step)


# ---- 2. the projector's lazy backward ------------------------------------------------------------------------------------------------
def _projector_model(I, hidden, use_id, text=None, cards=(2,)):
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel
    g = t.Generator().manual_seed(3)
    cat = t.stack([t.randint(0, c, (I,), generator=g) for c in cards], 1).to(DEV) if cards else None
    feats = ItemFeatures(cat, None, cardinalities=cards if cards else None, text=[c.to(DEV) for c in (text or ())])
    t.manual_seed(hidden)
    return PinSAGEModel(I, hidden, 1, features=feats, use_id=use_id).to(DEV)


@pytest.mark.parametrize("with_ids", [False, True], ids=["rows", "ids"])
@pytest.mark.parametrize("use_id,which", [(True, ("id",)), (True, ("cat",)), (True, ("id", "cat")), (False, ("cat",))],
                         ids=["id", "id-catlazy", "id-bothlazy", "noid"])
@pytest.mark.parametrize("hidden", [4, 20, 128])
def test_project_bwd_lazy(hidden, use_id, which, with_ids):
    """300 rows over a 2-value categorical column: two runs of about 150 references, across chunk borders, with chunks wholly
    inside a run.  All pairs null: mi_pinsage_project_bwd_f32's buffers bit for bit.  `which` slots lazy in ONE call (the id
    table alone, the column's table beside a dense id table, both; without an id table, the column's): p / m / v of each are the
    emulation over segsum_emulation's summed rows, its gradient buffer reads zero on the rows it consumed, and a slot left
    dense keeps the plain call's gradient and its table."""
    I = 300
    model = _projector_model(I, hidden, use_id)
    pr = model.projector
    gen = t.Generator().manual_seed(11 + hidden)
    ids = t.randint(0, I // 2, (300,), generator=gen) if with_ids else None
    rows = ids if with_ids else t.arange(I)
    gout = t.randn(300, hidden, generator=gen)
    params = pr.parameter_list()
    dev_ids = None if ids is None else ids.to(DEV)

    def buffers():
        return [t.full_like(p, SENTINEL) for p in params]

    plain = buffers()
    pr.project_backward(dev_ids, gout.to(DEV), plain)
    before = [p.detach().clone() for p in params]
    null = buffers()
    pr.project_backward_lazy(dev_ids, gout.to(DEV), null, [None] * len(params), (_lazy(1), _lazy(1)))
    assert all(t.equal(a, b) for a, b in zip(null, plain))
    assert all(t.equal(p, b) for p, b in zip(params, before))

    names = (["id"] if use_id else []) + ["cat"]                          # parameter_list() = [id table?] + [the column's table]
    assert len(names) == len(params)
    slot_of = {"cat": 0, "id": 1}                                         # segsum's slot order: the columns, then the id
    codes = [pr.x[:, 0].cpu().numpy()[rows.numpy()]] + ([rows.numpy()] if use_id else [])
    sums = E.segmented_sum(*E.projector_references(codes, gout.numpy()))
    assert max((np.concatenate(codes[:1]) == c).sum() for c in (0, 1)) > 2 * E.PIECE
    rng = np.random.default_rng(5)
    lazy_ks = [k for k, nm in enumerate(names) if nm in which]
    assert len(lazy_ks) == len(which)
    moments, start = [None] * len(params), {}
    for k in lazy_ks:
        m0 = (rng.standard_normal(tuple(params[k].shape)) * 0.1).astype(np.float32)
        v0 = (rng.random(tuple(params[k].shape)) * 0.01).astype(np.float32)
        start[k] = (m0, v0)
        moments[k] = (t.from_numpy(m0.copy()).to(DEV), t.from_numpy(v0.copy()).to(DEV))
    got = buffers()
    pr.project_backward_lazy(dev_ids, gout.to(DEV), got, moments, (_lazy(3), _lazy(3)))
    for k in lazy_ks:
        (m0, v0), (dm, dv) = start[k], moments[k]
        p, m, v = before[k].cpu().numpy().copy(), m0.copy(), v0.copy()
        _, touched = LE.update_from_sums(p, m, v, sums, slot_of[names[k]], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], 3)
        assert len(touched) and len(touched) < p.shape[0], names[k]
        assert _same_bits(params[k], p) and _same_bits(dm, m) and _same_bits(dv, v), names[k]
        rest = np.setdiff1d(np.arange(p.shape[0]), touched)
        assert _same_bits(params[k].detach().cpu().numpy()[rest], before[k].cpu().numpy()[rest]), names[k]
        assert _same_bits(dm.cpu().numpy()[rest], m0[rest]) and _same_bits(dv.cpu().numpy()[rest], v0[rest]), names[k]
        want_g = np.full(p.shape, SENTINEL, dtype=np.float32)
        want_g[touched] = 0.0                                             # consumed: reads (+)zero again
        assert _same_bits(got[k], want_g), names[k]
    for j in range(len(params)):
        if j not in lazy_ks:
            assert t.equal(got[j], plain[j]) and t.equal(params[j], before[j]), names[j]


# ---- 3. the text columns' lazy backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [20, 128])
def test_text_bwd_lazy(hidden):
    """Vocabulary 64 (63 = the pad id, in no bag), bag lengths 0 .. 12, 24 selected rows (with repeats) of 200 items, n_ref_max
    twice the true count: the padding keys sort last and never head a run.  Half of the tokens come from {0 .. 3}: runs across
    chunk borders."""
    from laplace_amd import _lib
    from laplace_amd.pinsage.model import TextColumn
    I, V, PAD = 200, 64, 63
    gen = t.Generator().manual_seed(hidden)
    ln = t.randint(0, 13, (I,), generator=gen)
    ln[::5] = 0
    tokens = t.where(t.rand(I, 12, generator=gen) < 0.5, t.randint(0, 4, (I, 12), generator=gen), t.randint(0, PAD, (I, 12), generator=gen))
    tokens[t.arange(12)[None, :] >= ln[:, None]] = PAD
    model = _projector_model(I, hidden, False, text=[TextColumn(tokens, ln, V, pad_id=PAD)], cards=())
    pr = model.projector
    ids = t.randint(0, I // 4, (24,), generator=gen)
    ids[3] = 0                                                            # an empty bag among the selected
    gout = t.randn(24, hidden, generator=gen)
    ptr, tok = pr.text_ptr_0.cpu().numpy(), pr.text_tok_0.cpu().numpy()
    keys, values = E.text_references([(ptr, tok)], ids.numpy(), gout.numpy())
    true_count = len(keys)
    assert true_count > E.PIECE and (keys == 0).sum() >= 2
    sums = E.segmented_sum(keys, values)
    table = pr.text_tables[0]
    before = table.detach().cpu().numpy().copy()
    rng = np.random.default_rng(9)
    m0 = (rng.standard_normal(before.shape) * 0.1).astype(np.float32)
    v0 = (rng.random(before.shape) * 0.01).astype(np.float32)
    dm, dv = t.from_numpy(m0.copy()).to(DEV), t.from_numpy(v0.copy()).to(DEV)
    gbuf = t.full_like(table, SENTINEL)
    L, b = _lib.lib(), pr.bind()
    n_ref_max = 2 * true_count
    ws = t.empty(int(L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(b.text), 24, n_ref_max)), dtype=t.uint8, device=DEV)
    gt, mt, vt = _lib.TextGradTables(), _lib.TextGradTables(), _lib.TextGradTables()
    gt[0], mt[0], vt[0] = gbuf.data_ptr(), dm.data_ptr(), dv.data_ptr()
    dg, dids = gout.to(DEV), ids.to(DEV)
    _lib.check(L.mi_pinsage_text_bwd_lazy_f32(ctypes.byref(b.text), gt, mt, vt, ctypes.byref(_lazy(2)), 24, dids.data_ptr(), dg.data_ptr(),
                                              hidden, n_ref_max, ws.data_ptr(), ws.numel(), _lib.current_stream()),
               "mi_pinsage_text_bwd_lazy_f32")
    assert int(ws[:8].view(t.int64).item()) == true_count
    p, m, v = before.copy(), m0.copy(), v0.copy()
    _, touched = LE.update_from_sums(p, m, v, sums, 0, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], 2)
    rest = np.setdiff1d(np.arange(V), touched)
    assert PAD in rest and len(rest) > 1 and len(touched) > 4            # the pad id and the tokens of unselected items only
    assert _same_bits(table, p) and _same_bits(dm, m) and _same_bits(dv, v)
    assert _same_bits(table.detach().cpu().numpy()[rest], before[rest]) and _same_bits(dm.cpu().numpy()[rest], m0[rest])
    want_g = np.full(before.shape, SENTINEL, dtype=np.float32)
    want_g[touched] = 0.0
    assert _same_bits(gbuf, want_g)
    # null pairs: the plain entry bit for bit
    plain, null = t.full_like(table, SENTINEL), t.full_like(table, SENTINEL)
    pr.project_backward(dids, dg, [plain])
    pr.project_backward_lazy(dids, dg, [null], [None], (_lazy(1), _lazy(1)))
    assert t.equal(plain, null) and _same_bits(table, p)


# ---- 4 - 6. the model ---------------------------------------------------------------------------------------------------------------------
_GRAPH = {}
N_ITEMS, HIDDEN, LAYERS, BATCH, LR = 200, 16, 2, 8, 3e-3


def _sampler(seed=11, batch=BATCH):
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U = 600
    if not _GRAPH:
        ei = S.generate(S.SyntheticSpec(U, N_ITEMS, 8000, seed=4, deg_min=1, deg_max=60, zipf_s=0.9))
        u, a = ei[0].numpy(), ei[1].numpy()
        _GRAPH["g"] = (AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, N_ITEMS))
    users, items = _GRAPH["g"]
    return PinSAGESampler(users, items, U, N_ITEMS, batch_size=batch, random_walk_length=2, num_layers=LAYERS, seed=seed)


def _model(kind, sparse_tables=True):
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel, TextColumn
    g = t.Generator().manual_seed(2)
    feats, use_id = None, True
    if kind == "id+cat+dense":
        cat = t.stack([t.randint(0, c, (N_ITEMS,), generator=g) for c in (7, 30)], 1).to(DEV)
        feats = ItemFeatures(cat, t.randn(N_ITEMS, 5, generator=g).to(DEV), cardinalities=(7, 30))
    elif kind in ("text", "id+text"):     # id+text: two lazy tables in one step, and no categorical table for the clear
        ln = t.randint(0, 9, (N_ITEMS,), generator=g)
        feats, use_id = ItemFeatures(text=[TextColumn(t.randint(0, 500, (N_ITEMS, 8), generator=g), ln, 500).to(DEV)]), kind != "text"
    t.manual_seed(1)
    model = PinSAGEModel(N_ITEMS, HIDDEN, LAYERS, features=feats, use_id=use_id, sparse_tables=sparse_tables).to(DEV)
    with t.no_grad():
        model.bias.normal_(0, 0.1)
    for cv in model.convs:
        cv.dropout.p = 0.0
    return model.train()


def _optimizers(model):
    return t.optim.Adam(model.dense_parameters(), lr=LR), t.optim.SparseAdam(model.sparse_parameters(), lr=LR)


def _autograd_step(model, opt, sopt, b):
    loss = model(b["seeds"], b["pos"], b["neg"], b["blocks"]).mean()
    opt.zero_grad(); sopt.zero_grad()
    loss.backward()
    opt.step(); sopt.step()
    return loss.detach()


def _changed(p, was):
    return set(t.nonzero((p.detach() != was).any(1)).view(-1).cpu().tolist())


def _agree(model, twin, what):
    worst = 0.0
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        worst = max(worst, float(((p - q).abs() - 1e-4 * q.abs()).max()))
    print(f"{what}: max(|a - b| - 1e-4 |b|) over every parameter = {worst:.3e} (allowed 2e-6)")
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert t.allclose(p, q, rtol=1e-4, atol=2e-6), (what, n, float((p - q).abs().max()))


KINDS = ["id", "id+cat+dense", "text", "id+text"]


@pytest.mark.parametrize("kind", KINDS)
def test_native_sparse_training_against_autograd(kind):
    from laplace_amd.pinsage.native import NativePinSAGEStep
    model = _model(kind)
    twin = copy.deepcopy(model)
    lazy = model.sparse_parameters()
    assert len(lazy) == (2 if kind == "id+text" else 1) and len(lazy) + len(model.dense_parameters()) == len(list(model.parameters()))
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in _model(kind, sparse_tables=False).named_parameters()]
    (opt, sopt), (opt_t, sopt_t) = _optimizers(model), _optimizers(twin)
    assert NativePinSAGEStep.unsupported_reason(model, opt, sopt) is None
    native, smp = NativePinSAGEStep(model, opt, sopt), _sampler()
    for i in range(5):
        b = smp.sample_batch()
        was = [(p.detach().clone(), q.detach().clone()) for p, q in zip(lazy, twin.sparse_parameters())]
        la = native.step(b)
        assert la is not None, native.declined
        lb = _autograd_step(twin, opt_t, sopt_t, b)
        print(f"{kind} step {i}: loss native {float(la):.7f} autograd {float(lb):.7f}")
        assert t.allclose(la.view(()), lb, rtol=1e-4, atol=2e-6), i
        for p, q, (wp, wq) in zip(lazy, twin.sparse_parameters(), was):
            moved, moved_t = _changed(p, wp), _changed(q, wq)
            assert moved == moved_t and 0 < len(moved) < p.shape[0], (i, len(moved), len(moved_t))
            assert p.grad is None
    _agree(model, twin, f"{kind}, 5 steps")
    for p, q in zip(lazy, twin.sparse_parameters()):
        st, st_t = sopt.state[p], sopt_t.state[q]
        assert type(st["step"]) is int and st["step"] == 5 == st_t["step"]
        for k in ("exp_avg", "exp_avg_sq"):                     # torch's own layout: dense, the table's shape
            assert st[k].shape == p.shape == st_t[k].shape and st[k].layout == t.strided
    assert all(float(opt.state[p]["step"]) == 5 for p in model.dense_parameters())


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_moves_between_native_and_torch(kind):
    """Three native steps; the SparseAdam / Adam state_dict()s load into fresh optimizers over a copy; two more steps native on
    one side, autograd on the other."""
    from laplace_amd.pinsage.native import NativePinSAGEStep
    model = _model(kind)
    opt, sopt = _optimizers(model)
    native, smp = NativePinSAGEStep(model, opt, sopt), _sampler(seed=13)
    for _ in range(3):
        assert native.step(smp.sample_batch()) is not None, native.declined
    twin = copy.deepcopy(model)
    opt_t, sopt_t = _optimizers(twin)
    opt_t.load_state_dict(copy.deepcopy(opt.state_dict()))
    sopt_t.load_state_dict(copy.deepcopy(sopt.state_dict()))
    # ... and the reverse: torch's own state into a fresh native step
    again = copy.deepcopy(model)
    opt_r, sopt_r = _optimizers(again)
    opt_r.load_state_dict(copy.deepcopy(opt_t.state_dict()))
    sopt_r.load_state_dict(copy.deepcopy(sopt_t.state_dict()))
    native_r = NativePinSAGEStep(again, opt_r, sopt_r, seed=native.seed)
    native_r.iteration = native.iteration
    for i in range(2):
        b = smp.sample_batch()
        la, lr_ = native.step(b), native_r.step(b)
        assert la is not None and lr_ is not None and float(la) == float(lr_)
        lb = _autograd_step(twin, opt_t, sopt_t, b)
        assert t.allclose(la.view(()), lb, rtol=1e-4, atol=2e-6), i
    _agree(model, twin, f"{kind}, 3 native + 2")
    assert all(t.equal(p, q) for p, q in zip(model.parameters(), again.parameters()))     # the reloaded native run: the same bits
    for p, q in zip(model.sparse_parameters(), twin.sparse_parameters()):
        assert sopt.state[p]["step"] == 5 == sopt_t.state[q]["step"]


@pytest.mark.parametrize("kind", ["id", "text"])
def test_second_step_after_a_larger_batch(kind):
    """A small batch, then a larger one (rows, workspaces and reference bounds regrow), then the small sampler again: still the
    autograd path's result."""
    from laplace_amd.pinsage.native import NativePinSAGEStep
    model = _model(kind)
    twin = copy.deepcopy(model)
    (opt, sopt), (opt_t, sopt_t) = _optimizers(model), _optimizers(twin)
    native = NativePinSAGEStep(model, opt, sopt)
    small, large = _sampler(seed=5, batch=4), _sampler(seed=6, batch=96)
    sizes = []
    for smp in (small, large, small):
        b = smp.sample_batch()
        sizes.append(int(b["blocks"][0]["src_ids"].numel()))
        la = native.step(b)
        assert la is not None, native.declined
        lb = _autograd_step(twin, opt_t, sopt_t, b)
        assert t.allclose(la.view(()), lb, rtol=1e-4, atol=2e-6)
    assert sizes[1] > 2 * sizes[0]
    _agree(model, twin, f"{kind}, regrown")


def test_optimizer_pairing_rules():
    from laplace_amd.pinsage.model import train_epoch
    from laplace_amd.pinsage.native import NativePinSAGEStep
    model = _model("id")
    opt, sopt = _optimizers(model)
    cases = [
        ((t.optim.Adam(model.parameters(), lr=LR), sopt), "dense_parameters"),
        ((opt, None), "sparse_optimizer"),
        ((opt, t.optim.Adam(model.sparse_parameters(), lr=LR)), "SparseAdam"),
        ((opt, t.optim.SparseAdam(model.sparse_parameters(), lr=LR, maximize=True)), "maximize"),
        ((opt, t.optim.SparseAdam([model.bias], lr=LR)), "sparse_parameters"),
    ]
    for (o, so), word in cases:
        why = NativePinSAGEStep.unsupported_reason(model, o, so)
        assert why is not None and word in why, (word, why)
        with pytest.raises(ValueError, match=word):
            NativePinSAGEStep(model, o, so)
    with pytest.raises(ValueError, match="data_parallel"):
        NativePinSAGEStep(model, opt, sopt, data_parallel=True)
    dense = _model("id", sparse_tables=False)
    assert dense.sparse_parameters() == [] and len(dense.dense_parameters()) == len(list(dense.parameters()))
    with pytest.raises(ValueError, match="no lazy tables"):
        NativePinSAGEStep(dense, t.optim.Adam(dense.parameters(), lr=LR), t.optim.SparseAdam([dense.proj.weight], lr=LR))
    with pytest.raises(ValueError, match="sparse_optimizer"):
        train_epoch(model, opt, _sampler(), 1)
    # keep_grads: nothing moves, the summed rows are exposed
    probe = NativePinSAGEStep(model, opt, sopt, keep_grads=True)
    before = [p.detach().clone() for p in model.parameters()]
    b = _sampler(seed=3).sample_batch()
    assert probe.step(b) is not None, probe.declined
    g = probe.table_grad(model.proj.weight)
    assert g.is_sparse and g.shape == model.proj.weight.shape and model.proj.weight.grad is None
    assert sorted(g.indices()[0].cpu().tolist()) == sorted(b["blocks"][0]["src_ids"].cpu().tolist())
    assert all(t.equal(p, q) for p, q in zip(model.parameters(), before)) and len(sopt.state[model.proj.weight]) == 3
    assert sopt.state[model.proj.weight]["step"] == 0


@pytest.mark.parametrize("kind", ["id", "text"])
def test_dense_models_train_as_before_around_a_lazy_run(kind):
    """sparse_tables=False with the unchanged call: two runs of the existing path, a lazy run between them in the same process —
    the same bits, and the same initial draws as the lazy model's."""
    from laplace_amd.pinsage.model import train_epoch
    runs = []
    for which in ("dense", "lazy", "dense"):
        model = _model(kind, sparse_tables=(which == "lazy"))
        if which == "lazy":
            opt, sopt = _optimizers(model)
            losses = train_epoch(model, opt, _sampler(seed=21), 4, sparse_optimizer=sopt)
            assert sopt.state[model.sparse_parameters()[0]]["step"] == 4          # every iteration went through the native step
        else:
            opt = t.optim.Adam(model.parameters(), lr=LR)
            losses = train_epoch(model, opt, _sampler(seed=21), 4)
            runs.append((losses, [p.detach().clone() for p in model.parameters()], [opt.state[p]["exp_avg"].clone() for p in model.parameters()]))
        assert len(losses) == 4 and all(np.isfinite(losses))
    (l0, p0, m0), (l1, p1, m1) = runs
    assert l0 == l1 and all(t.equal(a, b) for a, b in zip(p0, p1)) and all(t.equal(a, b) for a, b in zip(m0, m1))
    a, b = _model(kind, sparse_tables=False), _model(kind, sparse_tables=True)
    assert all(t.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
