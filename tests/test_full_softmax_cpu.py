"""No GPU: the full-catalogue softmax's twin (tests/full_softmax_twin.py) against a slot-by-slot restatement of the rule, the
condition under which the GPU tests' tolerances can be met in fp32, what the shared cases contain, and the argument checks
of the trainer, the ops and the C entry."""
import ctypes
import math
import os
import sys

import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_softmax_twin as T  # noqa: E402

LAMS = (0.0, 1e-2)


# ---------------------------------------------------------------------------- 1: the twin states the rule
def _slot_by_slot(c, lam):
    """Loss and gradients from the header's coefficient formulas, in float64 Python sums."""
    f, e = c["final"].double(), c["e0"].double()
    users, pos, B, U, I = c["users"].tolist(), c["pos"].tolist(), c["B"], c["U"], c["I"]
    gf, ge = t.zeros_like(f), t.zeros_like(e)
    loss = 0.0
    for b in range(B):
        logit = [float(f[users[b]] @ f[U + i]) for i in range(I)]
        mx = max(logit)
        total = sum(math.exp(v - mx) for v in logit)
        loss += (mx + math.log(total) - logit[pos[b]]) / B
        for i in range(I):
            coef = (math.exp(logit[i] - mx) / total - (1.0 if i == pos[b] else 0.0)) / B
            gf[users[b]] += coef * f[U + i]
            gf[U + i] += coef * f[users[b]]
        for node in (users[b], U + pos[b]):
            loss += lam * float(e[node] @ e[node])
            ge[node] += 2.0 * lam * e[node]
    return loss, gf, ge


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", [0, 1, 3, 8])
def test_twin_equals_the_rule_slot_by_slot(i, lam):
    c = T.cases()[i]
    loss, gf, ge = T.reference(i, lam)
    want, wf, we = _slot_by_slot(c, lam)
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want))
    assert float((gf - wf).abs().max()) <= 1e-12 and float((ge - we).abs().max()) <= 1e-12


def test_one_item_gives_no_main_term_and_no_gradient():
    c = T.cases()[8]
    assert c["I"] == 1
    loss, gf, _ = T.reference(8, 0.0)
    assert float(loss) == 0.0 and float(gf.abs().max()) == 0.0


def test_cases_are_the_listed_shapes_with_long_runs_and_every_item_row_live():
    assert [(c["B"], c["d"], c["U"], c["I"]) for c in T.cases()] == list(T.SHAPES) and len(T.SHAPES) == 9
    crossing = 0
    for c in T.cases():
        assert c["d"] % 4 == 0 and int(c["users"].max()) < c["U"] and int(c["pos"].max()) < c["I"]
        by_user = sorted(c["users"].tolist())               # the order of the segmented sum's reference list
        crossing += sum(by_user[p - 1] == by_user[p] for p in range(64, c["B"], 64))
    assert crossing >= 2                                    # a user's slot rows cross a border of 64-reference chunks
    c = T.cases()[0]
    _, gf, _ = T.reference(0, 0.0)
    named = set(c["pos"].tolist())
    unnamed = [i for i in range(c["I"]) if i not in named]
    assert unnamed and all(float(gf[c["U"] + i].abs().max()) > 0.0 for i in unnamed)   # dense over the items
    idle = [u for u in range(c["U"]) if u not in set(c["users"].tolist())]
    assert idle and float(gf[idle].abs().max()) == 0.0      # and sparse over the users


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_fp32_arithmetic_meets_the_project_tolerances_on_every_case(i, lam):
    """The tolerances of the GPU tests can be met in fp32: torch's own fp32 evaluation of the twin does, on every case, with
    an order of magnitude to spare (measured here: loss 1.2e-7 relative, gradients 5.4e-8 at the worst)."""
    c = T.cases()[i]
    want, wf, we = T.reference(i, lam)
    loss, gf, ge = T.twin(c["final"], c["e0"], c["U"], c["users"], c["pos"], lam, t.float32)
    print(f"case {i} lam={lam}: loss err {abs(float(loss) - float(want)):.3e}, "
          f"grad err {float((gf.double() - wf).abs().max()):.3e}")
    assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    assert t.allclose(gf.double(), wf, atol=1e-6, rtol=1e-4) and t.allclose(ge.double(), we, atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 2: argument checks
def _tiny_model():
    from laplace_amd.model.lightgcn import LightGCN
    return LightGCN(4, 5, 8, 1)


GOOD = dict(objective="softmax", sparse_batch=False, full_softmax=True)


@pytest.mark.parametrize("kw", [
    dict(GOOD, objective="reference"), dict(GOOD, objective="bpr"), dict(GOOD, negatives="popularity"),
    dict(GOOD, negatives="in_batch"), dict(GOOD, n_neg=4), dict(GOOD, reference_sampler_quirks=True), dict(GOOD, neg_range=4),
    dict(GOOD, logq_correction=True), dict(GOOD, sparse_batch=True), dict(objective="softmax", full_softmax=True)])
def test_trainer_refuses_bad_full_softmax_options_before_the_gpu(kw):
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(ValueError):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(neg_range=5), dict(logq_correction=False), dict(logq_correction=None),
                                dict(n_neg=1), dict(negatives="uniform"), dict(reorder=True)])
def test_trainer_accepts_the_valid_full_softmax_options_up_to_the_device_check(kw):
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **dict(GOOD, **kw))


def test_workspace_size_answers_without_a_gpu():
    from laplace_amd import _lib
    L = _lib.lib()
    sizes = [L.mi_full_softmax_workspace_bytes(b, 128, 100000) for b in (1, 33, 4096, 16384)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 2 * 16384 * 128 * 4                 # the user image and the slot gradient rows
    # row images and per-chunk partials only: no B x I term can hide below this (B x I x 4 bytes = 6.1 GiB)
    assert sizes[-1] < 16 * 16384 * 128 * 4 + 64 * 2 ** 20
    assert L.mi_full_softmax_workspace_bytes(64, 256, 1) > 0 and L.mi_full_softmax_workspace_bytes(64, 4, 2 ** 31 - 2) > 0
    for batch, d, n_items in ((0, 128, 1000), (-1, 128, 1000), (64, 0, 1000), (64, 30, 1000), (64, 260, 1000), (64, 2, 1000),
                              (64, 128, 0), (64, 128, -5), (64, 128, 2 ** 31 - 1), (64, 128, 2 ** 31), (2 ** 30, 128, 1000)):
        assert L.mi_full_softmax_workspace_bytes(batch, d, n_items) == 0, (batch, d, n_items)


def test_c_entry_checks_its_arguments_before_any_launch():
    from laplace_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, BAD_ARG, WORKSPACE = _lib.MI_ERR_UNSUPPORTED, _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    buf = (ctypes.c_int64 * 64)()
    ok = (ctypes.addressof(buf) + 15) // 16 * 16

    def run(batch=8, d=64, n_items=5, users=ok, pos=ok, final=ok, ldf=None, e0=ok, lde=None, loss=ok, g_final=None,
            reg_w=None, ws=ok, ws_bytes=0):
        return L.mi_full_softmax_fwd_bwd_f32(batch, d, 4, n_items, users, pos, final, d if ldf is None else ldf, e0,
                                             d if lde is None else lde, 1e-6, 1.0, 1.0, loss, g_final, d, reg_w, ws, ws_bytes,
                                             None)
    assert run() == WORKSPACE and run(g_final=ok, reg_w=ok) == WORKSPACE   # everything else in order
    for kw in (dict(users=None), dict(pos=None), dict(final=None), dict(e0=None), dict(loss=None), dict(ws=None),
               dict(batch=0), dict(batch=-3), dict(n_items=0), dict(n_items=-1),
               dict(final=ok + 4), dict(e0=ok + 8), dict(users=ok + 4), dict(loss=ok + 2), dict(ldf=60), dict(lde=66),
               dict(ws=ok + 8)):
        assert run(**kw) == BAD_ARG, kw
    for d in (30, 6, 260, 512):
        assert run(d=d) == UNSUPPORTED, d
    assert run(reg_w=ok) == UNSUPPORTED              # the loss-only form takes no reg_w
    assert run(n_items=2 ** 31 - 1) == _lib.MI_ERR_TOO_LARGE and run(batch=2 ** 30) == _lib.MI_ERR_TOO_LARGE
    big = L.mi_full_softmax_workspace_bytes(8, 64, 5)
    assert run(ws_bytes=big - 1) == WORKSPACE and run(g_final=ok, ws_bytes=big - 1) == WORKSPACE


def test_ops_check_width_and_shapes_first_and_refuse_cpu_tensors():
    from laplace_amd import ops
    from laplace_amd._lib import MiError
    from laplace_amd.utils.metrics_lightgcn import full_softmax_loss
    u, p = t.zeros(4, dtype=t.int64), t.zeros(4, dtype=t.int64)
    emb = t.zeros(9, 8)
    for d in (30, 6, 260):
        with pytest.raises(ValueError):
            ops.full_softmax_fwd_bwd(u, p, t.zeros(9, d), t.zeros(9, d), 4, 1e-6)
    with pytest.raises(ValueError):                  # the loss-only form takes no reg_w
        ops.full_softmax_fwd_bwd(u, p, emb, emb, 4, 1e-6, reg_w=t.zeros(9))
    with pytest.raises(ValueError):                  # no item row left
        ops.full_softmax_fwd_bwd(u, p, emb, emb, 9, 1e-6)
    with pytest.raises(ValueError):                  # pos: one per slot
        ops.full_softmax_fwd_bwd(u, p[:3], emb, emb, 4, 1e-6)
    with pytest.raises(MiError):                     # in range: the device check is next, no CPU fallback
        ops.full_softmax_fwd_bwd(u, p, emb, emb, 4, 1e-6)
    with pytest.raises(ValueError):
        full_softmax_loss(emb[:4], emb[4:], p[:3], emb[:4], emb[:4], 1e-6)
    with pytest.raises(MiError):
        full_softmax_loss(emb[:4], emb[4:], p, emb[:4], emb[:4], 1e-6)
