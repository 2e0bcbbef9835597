"""No GPU: the in-batch sampled softmax's twin (tests/inbatch_softmax_twin.py) against a slot-by-slot restatement of the
rule and against the M-negative sampled softmax it reduces to, what the shared kernel cases contain, and the argument
checks of the trainer, the ops and the C entry."""
import ctypes
import math
import os
import sys

import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inbatch_softmax_twin as T  # noqa: E402

LAMS = (0.0, 1e-2)


# ---------------------------------------------------------------------------- 1: the twin states the rule
def _slot_by_slot(c, lam, logq):
    """Loss and gradients from explicit candidate lists and the header's coefficient formulas, in float64 Python sums."""
    f, e = c["final"].double(), c["e0"].double()
    users, pos, B, G, U = c["users"].tolist(), c["pos"].tolist(), c["B"], c["G"], c["U"]
    lq = [0.0] * c["I"] if logq is None else logq.double().tolist()
    gf, ge = t.zeros_like(f), t.zeros_like(e)
    loss = 0.0
    for b in range(B):
        g0 = b // G * G
        cand = [j for j in range(g0, min(g0 + G, B))
                if j == b or (pos[j] != pos[b] and users[j] != users[b])]
        logit = {j: float(f[users[b]] @ f[U + pos[j]]) - lq[pos[j]] for j in cand}
        mx = max(logit.values())
        total = sum(math.exp(v - mx) for v in logit.values())
        if len(cand) > 1:
            loss += (mx + math.log(total) - logit[b]) / B
        for j in cand:
            coef = (math.exp(logit[j] - mx) / total - (1.0 if j == b else 0.0)) / B
            gf[users[b]] += coef * f[U + pos[j]]
            gf[U + pos[j]] += coef * f[users[b]]
        for node in (users[b], U + pos[b]):
            loss += lam * float(e[node] @ e[node])
            ge[node] += 2.0 * lam * e[node]
    return loss, gf, ge


@pytest.mark.parametrize("with_logq", [False, True])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", range(4))
def test_twin_equals_the_rule_slot_by_slot(i, lam, with_logq):
    c = T.cases()[i]
    loss, gf, ge = T.reference(i, lam, with_logq)
    want, wf, we = _slot_by_slot(c, lam, c["logq"] if with_logq else None)
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want))
    assert float((gf - wf).abs().max()) <= 1e-12 and float((ge - we).abs().max()) <= 1e-12


def test_distinct_ids_in_one_group_are_the_sampled_softmax_over_the_other_positives():
    """17 distinct users and items in one group: no mask, and slot b's 16 negatives are the other 16 positives."""
    from test_gpu_objectives import twin_loss
    c = T.cases()[1]
    B, U = c["B"], c["U"]
    assert B == 17 and c["G"] >= B and len(set(c["users"].tolist())) == B and len(set(c["pos"].tolist())) == B
    others = t.tensor([[j for j in range(B) if j != b] for b in range(B)])
    neg = c["pos"][others]                                   # [17, 16] item ids
    for lam in LAMS:
        loss, gf, ge = T.reference(1, lam, False)
        f = c["final"].double().requires_grad_(True)
        e = c["e0"].double().requires_grad_(True)
        u, p = c["users"], c["pos"]
        # the L2 term of the M-negative loss also counts the negatives' rows: taken off again
        want = twin_loss(f[u], e[u], f[U + p], e[U + p], f[U + neg], e[U + neg], lam, "softmax") \
            - lam * e[U + neg].pow(2).sum()
        want.backward()
        assert abs(float(loss) - float(want)) <= 1e-12
        assert float((gf - f.grad).abs().max()) <= 1e-12 and float((ge - e.grad).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------- 2: what the cases exercise
def test_cases_cover_masks_lonely_slots_and_long_runs():
    from collections import Counter
    own_item = own_user = lonely = 0
    longest = 0
    for c in T.cases():
        users, pos, B, G = c["users"].tolist(), c["pos"].tolist(), c["B"], c["G"]
        assert G % 32 == 0 and c["d"] % 4 == 0 and max(users) < c["U"] and max(pos) < c["I"]
        for b in range(B):
            g0 = b // G * G
            others = [j for j in range(g0, min(g0 + G, B)) if j != b]
            own_item += sum(pos[j] == pos[b] for j in others)
            own_user += sum(users[j] == users[b] and pos[j] != pos[b] for j in others)
            lonely += all(pos[j] == pos[b] or users[j] == users[b] for j in others)
        refs = Counter(users) + Counter(c["U"] + p for p in pos)
        longest = max(longest, max(refs.values()))
    print(f"masked pairs: {own_item} by item, {own_user} by user alone; {lonely} slots alone; longest run {longest}")
    assert own_item >= 1 and own_user >= 1      # a masked pair of each kind
    assert lonely >= 1                          # a slot whose only candidate is itself
    assert longest > 64                         # a node's references cross 64-reference chunks
    assert [(c["B"], c["G"], c["d"], c["U"], c["I"]) for c in T.cases()] == list(T.SHAPES) and len(T.SHAPES) == 8


@pytest.mark.parametrize("with_logq", [False, True])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_fp32_arithmetic_meets_the_project_tolerances_on_every_case(i, lam, with_logq):
    """The tolerances of the GPU tests can be met in fp32: torch's own fp32 evaluation of the twin does, on every case."""
    c = T.cases()[i]
    want, wf, we = T.reference(i, lam, with_logq)
    loss, gf, ge = T.twin(c["final"], c["e0"], c["U"], c["users"], c["pos"], c["G"], lam,
                          c["logq"] if with_logq else None, t.float32)
    print(f"case {i} lam={lam} logq={with_logq}: loss err {abs(float(loss) - float(want)):.3e}, "
          f"grad err {float((gf.double() - wf).abs().max()):.3e}")
    assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    assert t.allclose(gf.double(), wf, atol=1e-6, rtol=1e-4) and t.allclose(ge.double(), we, atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------- 3: argument checks
def _tiny_model():
    from laplace_amd.model.lightgcn import LightGCN
    return LightGCN(4, 5, 8, 1)


@pytest.mark.parametrize("kw", [
    dict(objective="reference"), dict(objective="bpr"), dict(), dict(objective="softmax", n_neg=4),
    dict(objective="softmax", reference_sampler_quirks=True), dict(objective="softmax", neg_range=4),
    dict(objective="softmax", in_batch_group=0), dict(objective="softmax", in_batch_group=33),
    dict(objective="softmax", in_batch_group=8192), dict(objective="softmax", in_batch_group=True),
    dict(objective="softmax", in_batch_group="1024")])
def test_trainer_refuses_bad_in_batch_options_before_the_gpu(kw):
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(ValueError):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, negatives="in_batch", **kw)


@pytest.mark.parametrize("kw", [dict(), dict(in_batch_group=32), dict(in_batch_group=4096), dict(neg_range=5),
                                dict(logq_correction=False), dict(logq_correction=True), dict(n_neg=1)])
def test_trainer_accepts_the_valid_in_batch_options_up_to_the_device_check(kw):
    from laplace_amd.trainer import NEGATIVES, LightGCNTrainer
    assert NEGATIVES == ("uniform", "popularity", "in_batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, negatives="in_batch",
                        objective="softmax", **kw)


def test_workspace_size_answers_without_a_gpu():
    from laplace_amd import _lib
    L = _lib.lib()
    sizes = [L.mi_inbatch_softmax_workspace_bytes(b, 128, 1024) for b in (1, 33, 4096, 16384)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 4 * 16384 * 128 * 4          # two row images and the 2B slot gradient rows
    assert L.mi_inbatch_softmax_workspace_bytes(64, 256, 32) > 0 and L.mi_inbatch_softmax_workspace_bytes(64, 4, 4096) > 0
    for batch, d, group in ((0, 128, 1024), (-1, 128, 1024), (64, 0, 1024), (64, 30, 1024), (64, 260, 1024), (64, 128, 0),
                            (64, 128, 16), (64, 128, 48), (64, 128, 8192), (2 ** 30, 128, 1024)):
        assert L.mi_inbatch_softmax_workspace_bytes(batch, d, group) == 0, (batch, d, group)


def test_c_entry_checks_its_arguments_before_any_launch():
    from laplace_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, BAD_ARG, WORKSPACE = _lib.MI_ERR_UNSUPPORTED, _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    buf = (ctypes.c_int64 * 64)()
    ok = (ctypes.addressof(buf) + 15) // 16 * 16

    def run(batch=8, group=32, d=64, users=ok, pos=ok, final=ok, ldf=None, e0=ok, lde=None, loss=ok, g_final=None,
            reg_w=None, node_map=None, logq=None, ws=ok, ws_bytes=0):
        return L.mi_inbatch_softmax_fwd_bwd_f32(batch, group, d, 4, users, pos, final, d if ldf is None else ldf, e0,
                                                d if lde is None else lde, 1e-6, 1.0, 1.0, loss, g_final, d, reg_w, node_map,
                                                logq, ws, ws_bytes, None)
    assert run() == WORKSPACE and run(g_final=ok, reg_w=ok, logq=ok) == WORKSPACE   # everything else in order
    for kw in (dict(users=None), dict(pos=None), dict(final=None), dict(e0=None), dict(loss=None), dict(ws=None),
               dict(batch=0), dict(batch=-3), dict(group=0), dict(group=16), dict(group=48), dict(group=8192),
               dict(final=ok + 4), dict(e0=ok + 8), dict(users=ok + 4), dict(logq=ok + 2), dict(ldf=60), dict(lde=66),
               dict(ws=ok + 8)):
        assert run(**kw) == BAD_ARG, kw
    for d in (30, 6, 260, 512):
        assert run(d=d) == UNSUPPORTED, d
    assert run(reg_w=ok) == UNSUPPORTED              # the loss-only form takes no reg_w
    big = L.mi_inbatch_softmax_workspace_bytes(8, 64, 32)
    assert run(ws_bytes=big - 1) == WORKSPACE and run(g_final=ok, ws_bytes=big - 1) == WORKSPACE


def test_ops_check_group_and_width_first_and_refuse_cpu_tensors():
    from laplace_amd import ops
    from laplace_amd._lib import MiError
    from laplace_amd.utils.metrics_lightgcn import in_batch_softmax_loss
    u, p = t.zeros(4, dtype=t.int64), t.zeros(4, dtype=t.int64)
    emb = t.zeros(9, 8)
    for group in (0, 33, 48, 8192, True, "1024", 64.0):
        with pytest.raises(ValueError):
            ops.inbatch_softmax_fwd_bwd(u, p, emb, emb, 4, 1e-6, group=group)
        with pytest.raises(ValueError):
            in_batch_softmax_loss(emb[:4], emb[:4], emb[:4], emb[:4], 1e-6, group=group)
    for d in (30, 6, 260):
        with pytest.raises(ValueError):
            ops.inbatch_softmax_fwd_bwd(u, p, t.zeros(9, d), t.zeros(9, d), 4, 1e-6)
    with pytest.raises(ValueError):                  # the loss-only form takes no reg_w
        ops.inbatch_softmax_fwd_bwd(u, p, emb, emb, 4, 1e-6, reg_w=t.zeros(9))
    with pytest.raises(MiError):                     # in range: the device check is next, no CPU fallback
        ops.inbatch_softmax_fwd_bwd(u, p, emb, emb, 4, 1e-6, group=32, logq=t.zeros(5))
    with pytest.raises(MiError):
        in_batch_softmax_loss(emb[:4], emb[:4], emb[:4], emb[:4], 1e-6, group=32)
