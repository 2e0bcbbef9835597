"""GPU: the native ranker step (mi_ranker_step_f32, the path bench.py times for the ranker configuration) over the table of
tests/ranker_step_cases.py — every twin launch of csrc/pairs.hpp against the two single launches it replaces, and both against
the op-by-op path and a float64 oracle.

For every case three copies of one model are driven over three batches: by NativeRankerStep as it is by default (twin launches
where the two sides share a kernel instantiation), by NativeRankerStep under LAPLACE_RANKER_AUX=1 (every pair as two single
launches on two streams, ordered by fork / join events) and, without dropout, by FusedRankerStep.  At every step:
  * the launches each executor reports (NativeRankerStep.last_launches) are the ones ranker_step_cases.expected_launches predicts:
    a launcher that always fell back, or never, fails here while every value below still agrees;
  * twin and single launches agree BIT FOR BIT on the loss, every gradient, the BatchNorm statistics, every updated parameter and
    both Adam moments — with dropout too: the masks are keyed on (seed, step, site), not on the launch form;
  * loss and gradients are bitwise FusedRankerStep's (p = 0), parameters and moments within the bounds of
    test_gpu_ranker.py::test_native_ranker_step_equals_the_fused_step;
  * loss, every gradient and the BatchNorm statistics against oracle/ranker_ref.py in float64 on the CPU — with dropout, under the
    masks tests/ranker_dropout_mirror.py computes for every site, which pins the mask of every element in the forward and in the
    backward.  Bounds: the project's own (tests/test_gpu_native_vs_oracle.py: loss 1e-5, gradients 2e-4 max|g| + 1e-6, statistics
    1e-5, the variance with rtol 1e-5 on top) as the floor; they were set at a width of 64, so each figure is allowed 8 times the distance of the SAME oracle run in
    float32 from its float64 run where that is more (the device sums in another order than torch's CPU kernels; a wrong lane,
    column or mask is off by orders of magnitude, not by a factor).  The distances are printed and recorded in the case table.
"""
import copy
import os
import sys

import pytest
import torch as t

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranker_dropout_mirror as DM  # noqa: E402
import ranker_step_cases as RC  # noqa: E402
from oracle import ranker_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = (0x5EED << 32) | 0x0DDBA11          # both halves of the key in use
NORMS = ("encoder_layer_norm_customer", "encoder_layer_norm_article")


def _copy_sharing_tables(model):
    twin = copy.deepcopy(model)
    twin.embedding_layers = model.embedding_layers       # frozen tables, shared
    return twin


def _oracle(model, first, dtype):
    ref = RR.ref_from_product(model, first.x_dict).to(dtype)
    for mods in ref.embedding_layers.values():           # a plain dict: .to() does not reach them
        for m in mods:
            m.to(dtype)
    return ref.train()


def _masks(case, shape, step, dtype):
    """The multiplier of every dropout site of one step, from the mirror; None without dropout."""
    if case.p <= 0:
        return None
    out = {}
    ins = RC.layer_inputs(case)
    for l in range(len(case.conv) - 1):
        for ti, n in enumerate((shape["n_c"], shape["n_a"])):
            out[DM.encoder_site(l, ti)] = t.from_numpy(DM.multiplier((n, ins[l][ti]), case.p, SEED, step, DM.encoder_site(l, ti))).to(dtype)
    width = 2 * case.C
    for j in range(case.dec_layers - 1):
        out[DM.decoder_site(j)] = t.from_numpy(DM.multiplier((shape["n_label"], width), case.p, SEED, step, DM.decoder_site(j))).to(dtype)
        width = case.dec_hidden
    return out


def _oracle_step(ref, model, batch, masks):
    """Loss, gradients and the BatchNorm statistics of one iteration of the oracle from the model's current weights and buffers."""
    from laplace_amd.utils.get_info import select_properties
    dtype = next(ref.parameters()).dtype
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ref.set_dropout_masks(masks)
    ref.zero_grad()
    x, ei, eli, y = select_properties(batch)
    out = ref({k: v.clone() for k, v in x.items()}, ei, eli)
    loss = t.nn.BCEWithLogitsLoss()(out, y.to(dtype))
    loss.backward()
    stats = {f"{bn}.{k}": getattr(getattr(ref, bn), k).detach().clone() for bn in NORMS for k in ("running_mean", "running_var")}
    counts = [int(getattr(ref, bn).num_batches_tracked) for bn in NORMS]
    return float(loss), {n: p.grad.detach().clone() for n, p in ref.named_parameters()}, stats, counts


def _distances(loss, grads, stats, want):
    """Of (loss, grads, stats) from the float64 oracle's, each as a FRACTION OF THE PROJECT'S BOUND for it
    (tests/test_gpu_native_vs_oracle.py): |loss - loss64| / 1e-5;  per tensor max|g - g64| / (2e-4 max|g64| + 1e-6) — the absolute
    term is what a bias in front of the BatchNorm needs, whose true gradient is exactly zero;  per statistic
    max(|s - s64| / (1e-5 + 1e-5 |s64|)) for the running variance and max|s - s64| / 1e-5 for the running mean."""
    l64, g64, s64 = want
    tol = lambda n: (1e-5 + 1e-5 * s64[n].abs()) if n.endswith("running_var") else 1e-5   # noqa: E731
    return (abs(loss - l64) / 1e-5,
            {n: float((grads[n].double().cpu() - g64[n]).abs().max()) / (2e-4 * float(g64[n].abs().max()) + 1e-6) for n in g64},
            {n: float(((stats[n].double().cpu() - s64[n]).abs() / tol(n)).max()) for n in s64})


def _assert_against_float64(case, tag, device, f32):
    """device, f32: _distances of the native step and of the float32 oracle.  Every figure of the device stays inside the
    project's bound (a fraction of at most 1) or inside 8 times the float32 oracle's own distance, whichever is more."""
    worst = lambda d: max(d.values())   # noqa: E731
    print(f"[{case.name}] {tag}: fractions of the bound — device loss {device[0]:.3f} grad {worst(device[1]):.3f} stat {worst(device[2]):.3f}   "
          f"float32 oracle loss {f32[0]:.3f} grad {worst(f32[1]):.3f} stat {worst(f32[2]):.3f}")
    assert device[0] <= max(1.0, 8 * f32[0]), (tag, "loss", device[0], f32[0])
    for n, d in device[1].items():
        assert d <= max(1.0, 8 * f32[1][n]), (tag, n, d, f32[1][n])
    for n, d in device[2].items():
        assert d <= max(1.0, 8 * f32[2][n]), (tag, n, d, f32[2][n])


def _state(model, opt):
    out = {f"p.{n}": p.detach() for n, p in model.named_parameters()}
    out.update({f"g.{n}": p.grad for n, p in model.named_parameters()})
    for n, p in model.named_parameters():
        out[f"m.{n}"], out[f"v.{n}"] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    for bn in NORMS:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            out[f"{bn}.{k}"] = getattr(getattr(model, bn), k)
    return out


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_twin_launches_single_launches_op_by_op_and_float64(case, monkeypatch):
    from laplace_amd.ranker_native import NativeRankerStep
    from laplace_amd.ranker_step import FusedRankerStep
    from laplace_amd.utils.get_info import select_properties
    batches = RC.make_batches(case)
    first = batches[0].to(DEV)
    model = RC.make_model(case, first, DEV)
    assert [tuple(tb.shape) for tb in model.embedding_layers["customer"]] == [(RC.CARDS[i], d) for i, d in enumerate(case.cust_dims)]
    m_aux, m_ops = _copy_sharing_tables(model), (_copy_sharing_tables(model) if case.p == 0 else None)
    opt, o_aux = t.optim.Adam(model.parameters(), lr=0.01), t.optim.Adam(m_aux.parameters(), lr=0.01)
    assert NativeRankerStep.unsupported_reason(model, opt) is None
    monkeypatch.delenv("LAPLACE_RANKER_AUX", raising=False)
    twin = NativeRankerStep(model, opt, seed=SEED)
    monkeypatch.setenv("LAPLACE_RANKER_AUX", "1")
    aux = NativeRankerStep(m_aux, o_aux, seed=SEED)
    monkeypatch.delenv("LAPLACE_RANKER_AUX")
    assert twin._aux is None and aux._aux is not None
    fused = o_ops = None
    if m_ops is not None:
        o_ops = t.optim.Adam(m_ops.parameters(), lr=0.01)
        fused = FusedRankerStep(m_ops, o_ops)
        m_ops.train()
    ref64, ref32 = _oracle(model, first, t.float64), _oracle(model, first, t.float32)
    names = [n for n, _ in model.named_parameters()]
    assert names == [n for n, _ in ref64.named_parameters()]
    model.train(); m_aux.train()
    for step, batch in enumerate(batches):
        shape = RC.batch_shape(batch)
        if case.isolated:   # mean over an empty row on both sides
            assert int(shape["deg_c"].min()) == 0 and int(shape["deg_a"].min()) == 0
        want = _oracle_step(ref64, model, batch, _masks(case, shape, step, t.float64))
        f32 = _oracle_step(ref32, model, batch, _masks(case, shape, step, t.float32))
        assert want[3] == f32[3]
        x, ei, eli, y = select_properties(batch.to(DEV))
        la = twin.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
        lb = aux.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
        # ---- which launch ran
        assert la is not None and lb is not None and twin.declined is None and aux.declined is None, (twin.declined, aux.declined)
        rows = (shape["n_c"], shape["n_a"])
        assert twin.last_launches == RC.expected_launches(case, False, rows), step
        assert aux.last_launches == RC.expected_launches(case, True, rows), step
        # ---- twin launches against single launches on two streams: bit for bit
        t.cuda.synchronize()
        assert t.equal(la, lb), (step, float(la), float(lb))
        sa, sb = _state(model, opt), _state(m_aux, o_aux)
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert t.equal(sa[k], sb[k]), (step, k)
        assert float(opt.state[next(model.parameters())]["step"]) == float(o_aux.state[next(m_aux.parameters())]["step"]) == step + 1
        # ---- the op-by-op path
        if fused is not None:
            lc = fused.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
            assert lc is not None and float(la) == float(lc), step
            sc = _state(m_ops, o_ops)
            for n in names:
                assert t.equal(sa[f"g.{n}"], sc[f"g.{n}"]), (step, n)
                assert float((sa[f"p.{n}"] - sc[f"p.{n}"]).abs().max()) <= 2e-6, (step, n)          # Adam: same update to rounding
                assert t.allclose(sa[f"m.{n}"], sc[f"m.{n}"], rtol=1e-5, atol=1e-9), (step, n)
                assert t.allclose(sa[f"v.{n}"], sc[f"v.{n}"], rtol=1e-5, atol=1e-12), (step, n)
            for bn in NORMS:
                for k in ("running_mean", "running_var", "num_batches_tracked"):
                    assert t.equal(sa[f"{bn}.{k}"], sc[f"{bn}.{k}"]), (step, bn, k)
            m_ops.load_state_dict(model.state_dict())           # cut the chain at rounding level, as that test does
            for p, q in zip(model.parameters(), m_ops.parameters()):
                for k in ("exp_avg", "exp_avg_sq"):
                    o_ops.state[q][k].copy_(opt.state[p][k])
        # ---- float64
        grads = {n: sa[f"g.{n}"] for n in names}
        stats = {k: sa[k] for k in want[2]}
        _assert_against_float64(case, f"step {step}", _distances(float(la), grads, stats, want[:3]),
                                _distances(f32[0], f32[1], f32[2], want[:3]))
        assert [int(sa[f"{bn}.num_batches_tracked"]) for bn in NORMS] == want[3]


@pytest.mark.parametrize("case", [c for c in RC.CASES if c.mirror], ids=lambda c: c.name)
def test_dropout_masks_are_the_mirrored_ones(case):
    """Learning rate zero, so nothing moves: the native step's loss and every gradient at two iterations of the dropout stream
    against the float64 oracle under the mirror's masks.  A site number off by one, a float4 index computed wrongly where C / 4 is
    no power of two, or a backward that regenerates another mask than the forward drew gives a gross mismatch: a fraction p of
    the elements of that site changes."""
    from laplace_amd.ranker_native import NativeRankerStep
    from laplace_amd.utils.get_info import select_properties
    batches = RC.make_batches(case, n=2, seed=1)
    first = batches[0].to(DEV)
    model = RC.make_model(case, first, DEV, seed=1)
    opt = t.optim.Adam(model.parameters(), lr=0.0)
    native = NativeRankerStep(model, opt, seed=SEED)
    ref64, ref32 = _oracle(model, first, t.float64), _oracle(model, first, t.float32)
    names = [n for n, _ in model.named_parameters()]
    model.train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for batch, iteration in zip(batches, (0, (1 << 32) + 5)):       # the step's low word is the counter: 2^32 + 5 draws as 5 does
        shape = RC.batch_shape(batch)
        want = _oracle_step(ref64, model, batch, _masks(case, shape, iteration, t.float64))
        f32 = _oracle_step(ref32, model, batch, _masks(case, shape, iteration, t.float32))
        x, ei, eli, y = select_properties(batch.to(DEV))
        native.iteration = iteration
        loss = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
        assert loss is not None, native.declined
        assert native.last_launches == RC.expected_launches(case, False, (shape["n_c"], shape["n_a"]))
        grads = {n: p.grad for n, p in model.named_parameters()}
        stats = {k: getattr(getattr(model, k.split(".")[0]), k.split(".")[1]) for k in want[2]}
        _assert_against_float64(case, f"iteration {iteration}", _distances(float(loss), grads, stats, want[:3]),
                                _distances(f32[0], f32[1], f32[2], want[:3]))
    for n, p in model.named_parameters():
        assert t.equal(p.detach(), before[n]), n
    assert names
