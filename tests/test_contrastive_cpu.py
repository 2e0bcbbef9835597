"""CPU: the restatement of the noise-view contrastive term (tests/contrastive_emulation.py) checked against itself — the
noise's range and independence, the contrast's analytic gradient against autograd and finite differences, its edge cases —
and every refusal of the trainer, the ops and the C entries that needs no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch as t

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import contrastive_emulation as E  # noqa: E402


# ---------------------------------------------------------------------------- 1: the noise
@pytest.mark.parametrize("d", [4, 36, 128, 256])
def test_uniforms_lie_in_the_unit_interval_and_noise_rows_have_unit_norm(d):
    u = E.uniforms(np.arange(300), d, 2, seed=11, step=3)
    assert u.dtype == np.float32 and u.shape == (300, d) and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal(u * np.float32(2.0 ** 24), np.round(u * np.float32(2.0 ** 24)))      # multiples of 2^-24: exact
    n = E.noise(np.arange(300), d, 2, seed=11, step=3)
    assert np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0).max() < 1e-14
    assert 0.4 < float(u.mean()) < 0.6


def test_an_all_zero_row_stays_zero_and_signs_are_kept():
    g = np.random.default_rng(0)
    y = g.standard_normal((9, 8))
    y[3] = 0.0
    y[5, 2] = -0.0
    x = E.perturb(y, 0.2, 1, seed=1, step=0)
    assert np.array_equal(x[3], np.zeros(8)) and x[5, 2] == 0.0
    assert np.array_equal(np.sign(x), np.sign(y))                     # u >= 0: the perturbation pushes away from zero
    moved = np.sqrt(((x - y) ** 2).sum(axis=1))
    assert np.all(moved <= 0.2 + 1e-12) and moved[0] > 0.0


def test_a_rows_noise_depends_on_its_id_alone():
    whole = E.noise(np.arange(70), 36, 1, seed=5, step=2)
    assert np.array_equal(E.noise(np.arange(10), 36, 1, seed=5, step=2), whole[:10])
    perm = np.random.default_rng(1).permutation(70)
    assert np.array_equal(E.noise(perm, 36, 1, seed=5, step=2), whole[perm])
    y = np.random.default_rng(2).standard_normal((70, 36))
    assert np.array_equal(E.perturb(y, 0.2, 1, 5, 2), E.perturb(y, 0.2, 1, 5, 2, row_ids=np.arange(70)))
    assert np.array_equal(E.perturb(y[perm], 0.2, 1, 5, 2, row_ids=perm), E.perturb(y, 0.2, 1, 5, 2)[perm])
    for other in (dict(layer=2), dict(step=3), dict(seed=6)):
        kw = dict(layer=1, seed=5, step=2)
        kw.update(other)
        assert not np.array_equal(E.noise(np.arange(70), 36, **kw), whole), other
    assert E.key(5, 2) != E.key(7, 1) and E.key(2 ** 64 - 1, 1) == ((0x7F4A7C15 - 1) & 0xFFFFFFFF, 0x9E3779B9)


# ---------------------------------------------------------------------------- 2: the contrast
@pytest.mark.parametrize("duplicated", [False, True])
@pytest.mark.parametrize("B,G,d", [(33, 32, 4), (96, 32, 64), (160, 64, 64)])
def test_analytic_gradient_is_autograd_of_the_twin_and_a_central_difference(B, G, d, duplicated):
    c = E.case(B, G, d, duplicated)
    loss, ga, gb = E.reference(B, G, d, duplicated)
    loss2, ga2, gb2 = E.contrast_analytic(c["a"], c["b"], c["ids"], c["tau"], G)
    assert abs(float(loss) - float(loss2)) < 1e-12
    assert t.allclose(ga, ga2, atol=1e-13, rtol=1e-10) and t.allclose(gb, gb2, atol=1e-13, rtol=1e-10)
    a64, b64, h = c["a"].double(), c["b"].double(), 1e-6
    for which, table, grad in (("a", a64, ga), ("b", b64, gb)):
        for slot, col in ((0, 0), (B // 2, d - 1), (B - 1, d // 2)):
            row = int(c["ids"][slot])
            up, down = table.clone(), table.clone()
            up[row, col] += h
            down[row, col] -= h
            args = (lambda x: (x, b64)) if which == "a" else (lambda x: (a64, x))
            fd = (E.contrast_loss(*args(up), c["ids"], c["tau"], G) - E.contrast_loss(*args(down), c["ids"], c["tau"], G)) / (2 * h)
            assert abs(float(fd) - float(grad[row, col])) <= 1e-8 + 1e-6 * abs(float(grad[row, col])), (which, slot, col)
    untouched = t.ones(E.N_ROWS, dtype=t.bool)
    untouched[c["ids"]] = False
    assert float(ga[untouched].abs().sum()) == 0.0 and float(gb[untouched].abs().sum()) == 0.0


def test_a_slot_alone_in_its_group_adds_nothing():
    g = t.Generator().manual_seed(3)
    a, b = t.randn(40, 8, generator=g).double(), t.randn(40, 8, generator=g).double()
    assert float(E.contrast_loss(a, b, t.tensor([4]), 0.15, 32)) == 0.0
    ids = t.arange(33)
    whole = E.contrast_loss(a, b, ids, 0.15, 32)
    first = E.contrast_loss(a, b, ids[:32], 0.15, 32)
    assert abs(float(whole) * 33 - float(first) * 32) < 1e-12                    # the 33rd slot, alone in group 2, adds 0
    same = E.contrast_loss(a, b, t.full((7,), 9), 0.15, 32)                      # every other candidate masked
    assert float(same) == 0.0


def test_duplicated_ids_are_masked_as_candidates_of_each_other():
    g = t.Generator().manual_seed(4)
    a, b = t.randn(10, 8, generator=g).double(), t.randn(10, 8, generator=g).double()
    ids = t.tensor([1, 2, 1, 3])
    p, q = E._normalise(a[ids]), E._normalise(b[ids])
    logit = p @ q.T / 0.15
    want = 0.0
    for s, cand in ((0, (0, 1, 3)), (1, (0, 1, 2, 3)), (2, (1, 2, 3)), (3, (0, 1, 2, 3))):
        want += float(t.logsumexp(logit[s, list(cand)], dim=0) - logit[s, s])
    assert abs(float(E.contrast_loss(a, b, ids, 0.15, 32)) - want / 4) < 1e-12
    # a node named twice weighs twice: its gradient is the sum over its slots
    _, ga, _ = E.contrast_twin(a, b, ids, 0.15, 32)
    assert float(ga[1].abs().max()) > 0.0 and float(ga[0].abs().max()) == 0.0


@pytest.mark.parametrize("duplicated", [False, True])
@pytest.mark.parametrize("d", E.WIDTHS)
@pytest.mark.parametrize("G", E.GROUPS)
@pytest.mark.parametrize("B", E.BATCHES)
def test_fp32_arithmetic_meets_the_project_tolerances_on_every_case(B, G, d, duplicated):
    """The tolerances of the GPU tests (the in-batch softmax's) can be met in fp32: torch's own fp32 twin does."""
    c = E.case(B, G, d, duplicated)
    want, wa, wb = E.reference(B, G, d, duplicated)
    loss, ga, gb = E.contrast_twin(c["a"], c["b"], c["ids"], c["tau"], G, t.float32)
    assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    assert t.allclose(ga.double(), wa, atol=1e-6, rtol=1e-4) and t.allclose(gb.double(), wb, atol=1e-6, rtol=1e-4)
    if duplicated and B > 1:
        assert len(set(c["ids"].tolist())) <= 5
    else:
        assert len(set(c["ids"].tolist())) == B


def test_perturbed_forward_reduces_to_the_plain_forward_without_noise():
    from oracle import lightgcn_ref as R
    g = t.Generator().manual_seed(5)
    U, I, K = 12, 9, 3
    u, i = t.randint(0, U, (60,), generator=g), t.randint(0, I, (60,), generator=g)
    row, col = R.bipartite_edges(u, i, U)
    e0 = t.randn(U + I, 8, generator=g).double()
    adj = E.adjacency(row, col, U + I, t.float64)
    f, x1, smallest = E.perturbed_forward(e0, adj, K, 0.0, 1, 0, 1)
    uf, _, itf, _ = R.lightgcn_forward(e0[:U], e0[U:], row, col, K, dtype=t.float64)
    assert t.allclose(f, t.cat([uf, itf]), atol=1e-14) and smallest > 0.0
    f2, x3, _ = E.perturbed_forward(e0, adj, K, 0.2, 1, 0, 3)
    assert float((f2 - f).abs().max()) > 1e-3 and x3.shape == e0.shape


# ---------------------------------------------------------------------------- 3: refusals that need no GPU
def _model(d=8, K=2):
    from laplace_amd.model.lightgcn import LightGCN
    return LightGCN(4, 5, d, K)


@pytest.mark.parametrize("kw,word", [
    (dict(K=0), "K = 0"), (dict(cl_layer=0), "cl_layer"), (dict(cl_layer=3), "cl_layer"), (dict(cl_layer=True), "cl_layer"),
    (dict(cl_eps=-0.1), "eps"), (dict(cl_tau=0.0), "tau"), (dict(cl_tau=-1.0), "tau"), (dict(cl_group=48), "group"),
    (dict(cl_group=16), "group"), (dict(cl_group=8192), "group"), (dict(d=260), "d ="), (dict(sparse_batch=True), "sparse_batch"),
    (dict(cl_weight=-1.0), "cl_weight"), (dict(cl_weight=float("nan")), "cl_weight")])
def test_trainer_refuses_bad_contrastive_options_before_the_gpu(kw, word):
    from laplace_amd.trainer import LightGCNTrainer
    kw = dict(kw)
    model = _model(d=kw.pop("d", 8), K=kw.pop("K", 2))
    opts = dict(cl_weight=0.1, sparse_batch=False)
    opts.update(kw)
    with pytest.raises(ValueError, match=word):
        LightGCNTrainer(model, None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **opts)


def test_trainer_refuses_the_default_step_form_and_an_odd_width():
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(ValueError, match="sparse_batch"):                # sparse_batch defaults to True
        LightGCNTrainer(_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, cl_weight=0.1)
    model = _model()
    model.embedding_dim = 6                                              # LightGCN itself refuses d % 4 != 0
    with pytest.raises(ValueError, match="d % 4"):
        LightGCNTrainer(model, None, None, lr=1e-3, Lambda=1e-6, batch_size=4, cl_weight=0.1, sparse_batch=False)


@pytest.mark.parametrize("kw", [dict(), dict(cl_layer=2), dict(cl_group=32), dict(cl_eps=0.0), dict(objective="softmax", n_neg=4),
                                dict(objective="softmax", negatives="in_batch"), dict(objective="softmax", full_softmax=True)])
def test_trainer_accepts_the_valid_contrastive_options_up_to_the_device_check(kw):
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LightGCNTrainer(_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, cl_weight=0.1, sparse_batch=False, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # cl_weight = 0: the other keywords are not looked at
        LightGCNTrainer(_model(K=0), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, cl_weight=0.0, cl_layer=7, cl_group=5)


def test_ops_check_their_arguments_first_and_refuse_cpu_tensors():
    from laplace_amd import ops
    from laplace_amd._lib import MiError
    from laplace_amd.utils.metrics_lightgcn import contrastive_loss
    ids, emb = t.zeros(4, dtype=t.int64), t.zeros(9, 8)
    for bad in (dict(tau=0.0), dict(tau=-0.1), dict(tau=0.15, group=48), dict(tau=0.15, group=True), dict(tau=float("inf"))):
        with pytest.raises(ValueError):
            ops.contrastive_fwd_bwd(ids, emb, emb, **bad)
        with pytest.raises(ValueError):
            contrastive_loss(emb[:4], emb[:4], ids, **bad)
    for d in (30, 6, 260):
        with pytest.raises(ValueError):
            ops.contrastive_fwd_bwd(ids, t.zeros(9, d), t.zeros(9, d), tau=0.15)
    with pytest.raises(ValueError):                                      # one gradient table without the other
        ops.contrastive_fwd_bwd(ids, emb, emb, tau=0.15, g_a=t.zeros(9, 8))
    with pytest.raises(MiError, match="no CPU fallback"):
        ops.contrastive_fwd_bwd(ids, emb, emb, tau=0.15, group=32)
    for bad in (dict(eps=-1.0), dict(eps=0.2, layer=-1), dict(eps=0.2, layer=True), dict(eps=float("nan"))):
        kw = dict(eps=0.2, layer=1, seed=0, step=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.perturb_rows(t.zeros(9, 8), **kw)
    for d in (6, 260):
        with pytest.raises(ValueError):
            ops.perturb_rows(t.zeros(9, d), eps=0.2, layer=1, seed=0, step=0)
    with pytest.raises(MiError, match="no CPU fallback"):
        ops.perturb_rows(t.zeros(9, 8), eps=0.2, layer=1, seed=0, step=0)


def test_workspace_size_answers_without_a_gpu():
    from laplace_amd import _lib
    L = _lib.lib()
    sizes = [L.mi_contrastive_workspace_bytes(b, 128, 1024) for b in (1, 33, 4096, 16384)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 4 * 16384 * 128 * 4                              # two row images and the 2B slot gradient rows
    for batch, d, group in ((0, 128, 1024), (64, 0, 1024), (64, 30, 1024), (64, 260, 1024), (64, 128, 16), (64, 128, 48),
                            (64, 128, 8192), (2 ** 30, 128, 1024)):
        assert L.mi_contrastive_workspace_bytes(batch, d, group) == 0, (batch, d, group)


def test_c_entries_check_their_arguments_before_any_launch():
    from laplace_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, BAD_ARG, WORKSPACE = _lib.MI_ERR_UNSUPPORTED, _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    buf = (ctypes.c_int64 * 64)()
    ok = (ctypes.addressof(buf) + 15) // 16 * 16

    def run(batch=8, group=32, d=64, ids=ok, a=ok, lda=None, b=ok, ldb=None, inv_tau=6.0, loss=ok, g_a=None, g_b=None,
            ldg=None, ws=ok, ws_bytes=0):
        return L.mi_contrastive_fwd_bwd_f32(batch, group, d, ids, a, d if lda is None else lda, b, d if ldb is None else ldb,
                                            inv_tau, loss, g_a, d if ldg is None else ldg, 1.0, g_b, d, 1.0, ws, ws_bytes, None)
    assert run() == WORKSPACE and run(g_a=ok, g_b=ok) == WORKSPACE       # everything else in order
    for kw in (dict(ids=None), dict(a=None), dict(b=None), dict(loss=None), dict(ws=None), dict(batch=0), dict(batch=-3),
               dict(group=0), dict(group=16), dict(group=48), dict(group=8192), dict(a=ok + 4), dict(b=ok + 8), dict(ids=ok + 4),
               dict(loss=ok + 2), dict(lda=60), dict(ldb=66), dict(ws=ok + 8), dict(inv_tau=0.0), dict(inv_tau=-1.0),
               dict(inv_tau=float("inf")), dict(g_a=ok, g_b=ok, ldg=60), dict(g_a=ok + 2, g_b=ok)):
        assert run(**kw) == BAD_ARG, kw
    for d in (30, 6, 260, 512):
        assert run(d=d) == UNSUPPORTED, d
    assert run(g_a=ok) == UNSUPPORTED and run(g_b=ok) == UNSUPPORTED     # both gradients, or neither
    big = L.mi_contrastive_workspace_bytes(8, 64, 32)
    assert run(ws_bytes=big - 1) == WORKSPACE and run(g_a=ok, g_b=ok, ws_bytes=big - 1) == WORKSPACE

    def perturb(n=8, d=64, x=ok, ldx=None, row_ids=None, eps=0.2, layer=1, addend=None, lda=None, S=None, lds=None):
        return L.mi_perturb_rows_f32(n, d, x, d if ldx is None else ldx, row_ids, eps, layer, 1, 2, addend,
                                     d if lda is None else lda, S, d if lds is None else lds, 1.0, None)
    other = ok + 256
    for kw in (dict(x=None), dict(n=-1), dict(d=0), dict(x=ok + 4), dict(ldx=60), dict(ldx=66), dict(eps=-0.5), dict(layer=-1),
               dict(addend=other), dict(S=ok), dict(S=other + 4), dict(S=other, lds=66), dict(S=other, addend=ok),
               dict(S=other, addend=other, lda=68), dict(S=other, addend=other + 64, lda=62), dict(row_ids=ok + 4)):
        assert perturb(**kw) == BAD_ARG, kw
    for d in (30, 6, 260, 512):
        assert perturb(d=d) == UNSUPPORTED, d
    assert perturb(n=0) == 0                                             # no rows: nothing to do, nothing launched
