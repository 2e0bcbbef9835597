"""GPU: the native PinSAGE iteration (mi_pinsage_step_f32, csrc/pinsage_exec.hip) and the item pass
(mi_pinsage_embed_items_f32, csrc/pinsage_infer.hip) against a float64 restatement of the reference's layers on the CPU
(tests/pinsage_step_refs.py) — no shared kernel, no shared CSR builder — on hand-built batches at the edges the sampler's
batches never reach: cases A-K of that file's table.  Tolerance: bound(x64, x32) = 8 max|x32 - x64| + 4 * 2^-24 max|x64| per
tensor, x32 the same formulas in float32 on the CPU; what a case makes exactly zero or exactly known is compared with ==.

Every comparison prints `[ratio] case | family | tensor err e32 ratio bound scale` (pytest -s) before it asserts.

Recorded on an MI355X, one run: the largest error / max|x32 - x64| per tensor family, and the largest error / bound.
    family          cases A-I           J (dropout)   K (compact rows)   largest error / bound
    loss            20.2 (I-L4)         3.7           4.7                0.44 (B-p1)
    layer weights    6.9 (A-h4 W0)      2.0           2.5                0.66 (A-h4 W0.weight)
    layer biases     8.5 (A-h4 Q0)      2.7           2.7                0.79 (A-h4 Q0.bias)
    table rows       1.9 (A-h128)       1.5           1.9                0.18
    scorer bias      1.0                0.9           1.0                0.11 (E)
    item pass        1.0 (hidden 124, 1 layer, T 1)                      0.09
Two ratios are above 8; neither moved the factor, and both tensors are inside bound() through its second term.
* The loss is ONE number: its float32 evaluation can land within a fraction of an ulp of the float64 value by chance (I-L4:
  6e-9 at a loss of 1.39, a twentieth of an ulp), so the ratio says nothing there.  The executor's loss is within 2.4 ulp of
  the float64 one in every case (B-p1 the largest): each margin is the difference of two dot products of rows of norm ~3,
  each rounded once per term by pin_score_kernel.
* Layer-0 gradients at hidden 4 (A-h4: Q0.bias 8.5, W0.weight / W0.bias 6.9).  With four columns every sum of the float32
  evaluation has 4 or 8 terms and its error is 1.4 ulp of the tensor's largest entry; the executor's is 12 ulp at the far end
  of the backward chain.  What it rounds and the float32 evaluation does not: pin_l2norm_fwd_kernel multiplies by
  inv = 1 / norm (two roundings; torch divides, one), so a row with a single live column comes out as 1 - 2^-24 where torch
  has exactly 1, and dh - h (h . dh) in pin_l2norm_bwd_kernel then leaves an ulp of dh in a column whose exact value is 0
  (rows with one or two live columns are common at hidden 4); the edge values w / max(sum w, 1) are rounded to float32
  before the SpMM; the bias gradients come out of the MFMA product against the ones column.  Every one of these is a
  correctly rounded float32 operation or a reordering; every other layer gradient of the run, hidden 8 and
  up, stays below 2.8.
The scorer bias of B-p1 is +-1 exactly in all three evaluations (e32 = 0: no ratio).
"""
import pytest
import torch as t

import pinsage_step_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _family(key):
    return {"loss": "loss", "proj": "table rows", "bias": "scorer bias"}.get(key) or ("layer weights" if key.endswith("weight") else "layer biases")


def _model(case, sparse=False):
    from laplace_amd.pinsage.model import PinSAGEModel
    P = case["params"]
    model = PinSAGEModel(case["n_items"], case["hidden"], len(P["layers"]), sparse_tables=sparse).to(DEV)
    with t.no_grad():
        model.proj.weight.copy_(P["proj"])
        model.bias.copy_(P["bias"])
        for cv, (qw, qb, ww, wb) in zip(model.convs, P["layers"]):
            cv.Q.weight.copy_(qw); cv.Q.bias.copy_(qb); cv.W.weight.copy_(ww); cv.W.bias.copy_(wb)
    for cv in model.convs:
        cv.dropout.p = case["p"]
    model.train()
    return model


def _stepper(model, sparse=False, keep_grads=True):
    from laplace_amd.pinsage.native import NativePinSAGEStep
    if sparse:
        opt, sp = t.optim.Adam(model.dense_parameters(), lr=3e-3), t.optim.SparseAdam(model.sparse_parameters(), lr=3e-3)
        return NativePinSAGEStep(model, opt, sp, seed=R.EXEC_SEED, keep_grads=keep_grads), opt
    opt = t.optim.Adam(model.parameters(), lr=3e-3)
    return NativePinSAGEStep(model, opt, seed=R.EXEC_SEED, keep_grads=keep_grads), opt


def _grads(model, step, sparse):
    g = {"proj": step.table_grad(model.proj.weight).to_dense() if sparse else model.proj.weight.grad, "bias": model.bias.grad}
    for l, cv in enumerate(model.convs):
        g.update({"Q%d.weight" % l: cv.Q.weight.grad, "Q%d.bias" % l: cv.Q.bias.grad, "W%d.weight" % l: cv.W.weight.grad,
                  "W%d.bias" % l: cv.W.bias.grad})
    return {k: v.detach().double().cpu() for k, v in g.items()}


def _compare(label, got_loss, got, r64, r32, only=None):
    """bound() on the loss and every gradient; structural zeros with ==.  Every figure is printed before it is asserted."""
    failures = []
    for key, x64, x32 in R.compared(r64, r32):
        if only is not None and key not in only:
            continue
        x = t.as_tensor(got_loss, dtype=t.float64).reshape(x64.shape) if key == "loss" else got[key].reshape(x64.shape)
        err, e32 = float((x - x64).abs().max()), float((x32 - x64).abs().max())
        if R.structural_zero(x64, x32):
            print(f"[exact] {label} {key} max|x| {float(x.abs().max()):.3e}")
            if float(x.abs().max()) != 0.0:
                failures.append((key, "not exactly zero", float(x.abs().max())))
            continue
        tol = R.bound(x64, x32)
        print(f"[ratio] {label} | {_family(key)} | {key} err {err:.3e} e32 {e32:.3e} ratio {err / e32 if e32 else float('inf'):.2f} "
              f"bound {tol:.3e} scale {float(x64.abs().max()):.3e}")
        if not err <= tol:
            failures.append((key, err, tol))
    assert not failures, (label, failures)


def _run(name, sparse=False, iterations=(0,)):
    outs = []
    case = R.build_case(name)
    model = _model(case, sparse)
    step, _ = _stepper(model, sparse)
    batch = R.batch_to(case["batch"], DEV)
    for it in iterations:
        assert step.iteration == it
        loss = step.step(batch)
        assert loss is not None, step.declined
        outs.append((float(loss), _grads(model, step, sparse)))
    return case, outs


def _assert_all_zero(label, grads):
    bad = {k: float(v.abs().max()) for k, v in grads.items() if float(v.abs().max()) != 0.0}
    print(f"[exact] {label} every gradient == 0: {not bad}")
    assert not bad, (label, bad)


PLAIN = [n for n in R.CASES if R.CASES[n][0].get("exact") is None and not n.startswith("J")]


def test_table_and_library_agree_on_the_layer_limit():
    from laplace_amd import _lib
    assert R.MAX_LAYERS == _lib.MI_PINSAGE_MAX_LAYERS


@pytest.mark.parametrize("name", PLAIN)
def test_step_against_float64(name):
    """Cases A, B, C(ii), F, G, H, I: loss and every gradient within bound()."""
    case, [(loss, grads)] = _run(name)
    _, r64, r32 = R.evaluate_case(name)
    _compare(name, loss, grads, r64, r32)
    if name == "F-i":        # out of every pair, no edge in or out: nothing reaches the three zero rows
        rows = case["batch"]["seeds"][:3]
        assert float(grads["proj"][rows].abs().max()) == 0.0
    if name == "F-ii":       # rows of norm 0 in live pairs: only the h_dst_final term reaches their table rows
        rows = case["batch"]["seeds"][:3]
        assert float(grads["proj"][rows].abs().max()) > 0.0


def test_step_declines_more_than_1024_pairs():
    """Case B, n_pairs = 1025: beyond the score gradient's pair list — declined before anything is enqueued."""
    case = R.build_case("B-p1024")
    model = _model(case)
    step, opt = _stepper(model, keep_grads=False)
    b = case["batch"]
    u, v, w = (t.cat([x, x[:1]]) for x in (b["pos"][0], b["pos"][1], b["neg"][1]))
    batch = R.batch_to(R.make_batch(b["seeds"], b["blocks"], (u, v, w)), DEV)
    assert batch["pos"][0].numel() == 1025
    before = [p.detach().clone() for p in model.parameters()]
    assert step.step(batch) is None
    assert "UNSUPPORTED" in step.declined and "shape" in step.declined
    assert all(t.equal(x, p) for x, p in zip(before, model.parameters()))
    for p in model.parameters():
        st = opt.state.get(p, {})
        assert float(st.get("step", 0.0)) == 0.0
        assert all(float(st[k].abs().max()) == 0.0 for k in ("exp_avg", "exp_avg_sq") if k in st)
    ok = R.batch_to(b, DEV)                                   # the same executor takes 1024 right after
    assert step.step(ok) is not None, step.declined


@pytest.mark.parametrize("name", ["C-i", "C-iii"])
def test_degenerate_pairs_cancel_bit_for_bit(name):
    """tail == negative in every pair: every margin is 1.0f, the loss is exactly 1 and the +g x / -g x pairs cancel exactly
    (g = 1 / 64 and 1: powers of two)."""
    case, [(loss, grads)] = _run(name)
    print(f"[exact] {name} loss {loss!r}")
    assert loss == 1.0
    _assert_all_zero(name, grads)


def test_all_pairs_dead():
    """Case D: loss 0, every gradient 0; then one full step (Adam step 1) moves nothing."""
    case, [(loss, grads)] = _run("D")
    print(f"[exact] D loss {loss!r}")
    assert loss == 0.0
    _assert_all_zero("D", grads)
    model = _model(case)
    step, opt = _stepper(model, keep_grads=False)
    before = [p.detach().clone() for p in model.parameters()]
    loss = step.step(R.batch_to(case["batch"], DEV))
    assert loss is not None and float(loss) == 0.0
    for x, p in zip(before, model.parameters()):
        assert t.equal(x.view(t.int32), p.detach().view(t.int32))                   # bitwise
        st = opt.state[p]
        assert float(st["step"]) == 1.0
        assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0
    assert float(model.proj.weight.grad.abs().max()) == 0.0 and float(model.bias.grad.abs().max()) == 0.0


def test_margin_of_exactly_zero_is_active():
    """Case E: every margin is exactly 0.  The hinge is clamp(min=0), whose gradient torch passes at the bound: d bias is
    +k / n_pairs on a negative and -k / n_pairs on a tail that ends k pairs; the loss and everything else are exactly 0."""
    case, [(loss, grads)] = _run("E")
    _, r64, r32 = R.evaluate_case("E")
    print(f"[exact] E loss {loss!r}")
    assert loss == 0.0
    b = case["batch"]
    n_pairs, n_items = b["pos"][0].numel(), case["n_items"]
    want = t.zeros(n_items, dtype=t.float64)
    want.index_add_(0, b["seeds"][b["neg"][1]], t.full((n_pairs,), 1.0 / n_pairs, dtype=t.float64))
    want.index_add_(0, b["seeds"][b["pos"][1]], t.full((n_pairs,), -1.0 / n_pairs, dtype=t.float64))
    assert float((want - r64["grads"]["bias"][:, 0]).abs().max()) <= 1e-15 and float(want.abs().max()) > 0
    _compare("E", loss, grads, r64, r32, only=("bias",))
    _assert_all_zero("E", {k: v for k, v in grads.items() if k != "bias"})


@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith("J")])
def test_dropout_masks_at_every_site(name):
    """Case J: two consecutive steps on one batch against the reference with the Philox masks of iteration 0 and 1 — the four
    launch sites (forward dropout, the concatenation's, its backward in place, the merge's) must regenerate the same masks."""
    case, outs = _run(name, iterations=(0, 1))
    for it, (loss, grads) in enumerate(outs):
        _, r64, r32 = R.evaluate_case(name, it)
        _compare(f"{name}/it{it}", loss, grads, r64, r32)
    assert outs[0][0] != outs[1][0]


@pytest.mark.parametrize("name", R.K_CASES)
def test_compact_rows_mode(name):
    """Case K: a sparse_tables model — the executor hands the table and bias gradients back compactly (rows_out / bias_out)."""
    its = (0, 1) if name.startswith("J") else (0,)
    case, outs = _run(name, sparse=True, iterations=its)
    for it, (loss, grads) in enumerate(outs):
        _, r64, r32 = R.evaluate_case(name, it)
        _compare(f"K:{name}/it{it}", loss, grads, r64, r32)


# ------------------------------------------------------------------------------------------------------------- the item pass
_GRAPH = {}


def _sampler(T, layers):
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.sampler import PinSAGESampler
    if not _GRAPH:
        U, I_touched, I = 600, 250, 300                      # items 250 .. 299: isolated
        ei = S.generate(S.SyntheticSpec(U, I_touched, 5000, seed=7, deg_min=1, deg_max=60, zipf_s=0.9))
        u, a = ei[0].numpy(), ei[1].numpy()
        _GRAPH["g"] = (AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, I), U, I)
    users, items, U, I = _GRAPH["g"]
    return PinSAGESampler(users, items, U, I, batch_size=32, num_neighbors=T, num_layers=layers, seed=11)


@pytest.mark.parametrize("T", [1, 16])
@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("hidden", [4, 8, 20, 68, 124])
def test_item_pass_against_float64(hidden, layers, T):
    """embed_items against get_repr's forward in float64 over sample_blocks(ids, step) for batches of 97 ids; group sizes 1
    (hidden 4), 5 of 8 lanes (20), 17 of 32 (68), 31 of 32 (124); T = 16 is the kernel's limit.  The model seed is the first
    whose data pass the relu guard (the guard reads the two CPU evaluations only)."""
    from laplace_amd.pinsage.native import embed_items
    smp = _sampler(T, layers)
    n_items, step = 300, 3
    ids = t.arange(n_items, device=DEV)
    blocks = [[{k: (x.cpu() if isinstance(x, t.Tensor) else x) for k, x in b.items()} for b in smp.sample_blocks(chunk, step)]
              for chunk in ids.split(97)]
    for model_seed in range(16):
        params = R.make_item_params(t.Generator().manual_seed(1000 * hidden + 10 * layers + model_seed), n_items, hidden, layers)
        ev = [(R.reference_forward(params, bl, t.float64), R.reference_forward(params, bl, t.float32)) for bl in blocks]
        pre64 = [x for (h64, p64), _ in ev for x in p64]
        pre32 = [x for _, (h32, p32) in ev for x in p32]
        zero = t.zeros(1, dtype=t.float64)
        ok, worst = R.guard(pre64, pre32, zero, zero)
        if ok:
            break
    assert ok, worst
    x64, x32 = t.cat([e[0][0] for e in ev]), t.cat([e[1][0] for e in ev])
    case = {"params": params, "n_items": n_items, "hidden": hidden, "p": 0.0}
    model = _model(case)
    model.eval()
    with t.no_grad():
        out = embed_items(model, smp, step)
    assert out is not None and out.shape == (n_items, hidden)
    out = out.double().cpu()
    err, e32, tol = float((out - x64).abs().max()), float((x32 - x64).abs().max()), R.bound(x64, x32)
    print(f"[ratio] item-h{hidden}-L{layers}-T{T} | item pass | out err {err:.3e} e32 {e32:.3e} ratio {err / e32:.2f} bound {tol:.3e} "
          f"model seed {model_seed}")
    assert err <= tol
    # the isolated rows: proj + the layers over [0, h], written out
    iso = {}
    for dtype in (t.float64, t.float32):
        proj = params["proj"][250:300].to(dtype)
        h = proj
        for _, _, ww, wb in params["layers"]:
            z = t.relu(t.cat([t.zeros_like(h), h], 1) @ ww.to(dtype).T + wb.to(dtype))
            nz = z.norm(2, 1, keepdim=True)
            h = z / t.where(nz == 0, t.ones_like(nz), nz)
        iso[dtype] = (proj + h).double()
    assert float((x64[250:] - iso[t.float64]).abs().max()) <= 1e-12       # the blocks really left them alone
    err_iso, tol_iso = float((out[250:] - iso[t.float64]).abs().max()), R.bound(iso[t.float64], iso[t.float32])
    print(f"[ratio] item-h{hidden}-L{layers}-T{T} | item pass | isolated err {err_iso:.3e} bound {tol_iso:.3e}")
    assert err_iso <= tol_iso
