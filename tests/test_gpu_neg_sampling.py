"""GPU: popularity-weighted negatives (mi_sample_bpr_batch_pop) bit for bit against the numpy mirror of
tests/neg_sampling_emulation.py, the logQ-corrected softmax (mi_rank_loss_fwd_bwd_lq_f32) against its float64 twin, and
the trainer with negatives="popularity".

Tolerances are those of tests/test_gpu_objectives.py for the same quantities: loss 1e-6 * max(1, |loss|), gradients atol
1e-6 / rtol 1e-4, ten training steps <= 1e-4 on the embeddings, step forms within 1e-6 on the loss.  Nothing statistical
runs here: the frequencies of the rule are checked on the mirror (tests/test_neg_sampling_cpu.py) and the kernel has to
equal the mirror."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as t

import neg_sampling_emulation as E
from oracle import lightgcn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 0xDEADBEEFCAFE


def _ops():
    from laplace_amd import ops
    return ops


def _loss_close(got, want):
    return abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


# ---------------------------------------------------------------------------- 4: sampler vs the mirror
_GRAPH = {}


def _graph():
    """200 users x 90 items, 3000 edges by _sampler_graph()'s recipe (tests/test_gpu_objectives.py); then two items lose
    all their edges (weight 0) and one user is given every one of the 8 heaviest items (the rejection path)."""
    if not _GRAPH:
        from laplace_amd.interactions import Interactions
        U, I, n_edges = 200, 90, 3000
        g = t.Generator().manual_seed(3)
        keys = t.randperm(U * I, generator=g)[:n_edges]
        zero = (17, 60)
        keys = keys[~t.isin(keys % I, t.tensor(zero))]
        heavy = t.argsort(t.bincount(keys % I, minlength=I), descending=True, stable=True)[:8]
        fan = 5
        keys = t.unique(t.cat([keys, fan * I + heavy]))
        ei = t.stack([keys // I, keys % I])
        rowptr, col_s, _ = R.sparse_tensor_csr(ei[0], ei[1], U, I)
        _GRAPH.update(U=U, I=I, ei=ei, inter=Interactions(ei.to(DEV), U, I), rowptr=rowptr.numpy(), col=col_s.numpy(),
                      degree=t.bincount(ei[1], minlength=I), zero=zero, fan=fan, heavy=heavy)
    return _GRAPH


def _held(ei, I, users, items):
    """[B, M] mask: items[b, m] is one of users[b]'s items."""
    keys = t.sort(ei[0] * I + ei[1])[0]
    k = (users[:, None] * I + items).reshape(-1)
    at = t.searchsorted(keys, k).clamp(max=keys.numel() - 1)
    return (keys[at] == k).reshape(items.shape)


@pytest.mark.parametrize("power", [0.75, 1.0])
def test_sampler_bit_exact_vs_mirror(power):
    ops, G = _ops(), _graph()
    r, roe, I = G["inter"].csr(), G["inter"].row_of_edge(), G["I"]
    tab = ops.negative_table(G["degree"], power, device=DEV)
    cum = E.cum_u32(tab)
    assert tab.n_items == I and tab.cum.is_cuda and tab.logq.is_cuda
    for step in (0, 1, 12345678901):
        ou, op_, _ = ops.sample_bpr_batch(r, roe, 256, I, seed=SEED, step=step)
        one = None
        for n_neg in (1, 3, 16):
            us, ps, ns = ops.sample_bpr_batch(r, roe, 256, I, seed=SEED, step=step, n_neg=n_neg, table=tab)
            assert tuple(ns.shape) == ((256,) if n_neg == 1 else (256, n_neg))
            assert t.equal(us, ou) and t.equal(ps, op_)             # the uniform sampler's edge stream
            ns2 = ns.reshape(256, n_neg)
            one = ns2[:, 0].clone() if n_neg == 1 else one
            assert t.equal(ns2[:, 0], one)                          # column 0 is the n_neg = 1 draw
            wu, wp, wn = E.sample(G["rowptr"], G["col"], 256, n_neg, cum, SEED, step)
            assert np.array_equal(us.cpu().numpy(), wu) and np.array_equal(ps.cpu().numpy(), wp)
            assert np.array_equal(ns2.cpu().numpy(), wn), (power, step, n_neg)
            again = ops.sample_bpr_batch(r, roe, 256, I, seed=SEED, step=step, n_neg=n_neg, table=tab)
            assert all(t.equal(a, b) for a, b in zip((us, ps, ns), again))    # two calls, equal bits


def test_sampler_never_draws_user_items_or_zero_weight_items():
    ops, G = _ops(), _graph()
    r, roe, I = G["inter"].csr(), G["inter"].row_of_edge(), G["I"]
    tab = ops.negative_table(G["degree"], 0.75, device=DEV)
    us, ps, ns = (x.cpu() for x in ops.sample_bpr_batch(r, roe, 20000, I, seed=1, step=2, n_neg=16, table=tab))
    assert bool(_held(G["ei"], I, us, ps[:, None]).all())
    assert not bool(_held(G["ei"], I, us, ns).any())
    assert int(ns.min()) >= 0 and int(ns.max()) < I
    assert not bool(t.isin(ns, t.tensor(G["zero"])).any())
    fan = us == G["fan"]                                            # the user who holds the 8 heaviest items drew others
    assert int(fan.sum()) > 0 and not bool(t.isin(ns[fan], G["heavy"]).any())
    assert float((ns[:, 0] != ns[:, 1]).float().mean()) > 0.9      # the columns are independent draws
    wu, wp, wn = E.sample(G["rowptr"], G["col"], 20000, 16, E.cum_u32(tab), 1, 2)
    assert np.array_equal(ns.numpy(), wn)
    # edges_in_order and caller-provided outputs
    n_edges = G["ei"].shape[1]
    out = (t.empty(n_edges, dtype=t.int64, device=DEV), t.empty(n_edges, dtype=t.int64, device=DEV),
           t.empty(n_edges, 4, dtype=t.int64, device=DEV))
    got = ops.sample_bpr_batch(r, roe, n_edges, I, seed=5, step=0, edges_in_order=True, n_neg=4, out=out, table=tab)
    old = ops.sample_bpr_batch(r, roe, n_edges, I, seed=5, step=0, edges_in_order=True)
    assert got[2] is out[2] and t.equal(out[0], old[0]) and t.equal(out[1], old[1])
    wu, wp, wn = E.sample(G["rowptr"], G["col"], n_edges, 4, E.cum_u32(tab), 5, 0, edges_in_order=True)
    assert np.array_equal(out[0].cpu().numpy(), wu) and np.array_equal(out[2].cpu().numpy(), wn)
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(r, roe, 256, I - 1, seed=1, step=0, table=tab)
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(r, roe, 256, I, seed=1, step=0, table=tab, quirk=True)


# ---------------------------------------------------------------------------- 5: ends of the search
def _far_graph():
    """_graph() with every item id moved up by 1000, under a catalogue wide enough for the planted tables: the users
    hold none of the items the tables weigh, so nothing is rejected."""
    from laplace_amd.interactions import Interactions
    G = _graph()
    ei = t.stack([G["ei"][0], G["ei"][1] + 1000])
    I = 140000
    rowptr, col_s, _ = R.sparse_tensor_csr(ei[0], ei[1], G["U"], I)
    return Interactions(ei.to(DEV), G["U"], I), rowptr.numpy(), col_s.numpy()


def _planted(which):
    if which == "zeros":
        return np.array([0, 0, 5, 0, 1, 0, 0], dtype=np.int64)
    if which == "one":
        return np.array([3], dtype=np.int64)
    q = np.zeros(131073, dtype=np.int64)
    q[[0, 65536, 131072]] = 1
    return q


@pytest.mark.parametrize("which", ["zeros", "one", "depth17"])
def test_search_ends(which):
    ops = _ops()
    inter, rowptr, col = _far_graph()
    q = _planted(which)
    tab = ops.negative_table_from_counts(q, DEV)
    n = int(q.shape[0])
    allowed = set(np.nonzero(q)[0].tolist())
    seen = set()
    for step in (0, 3):
        us, ps, ns = ops.sample_bpr_batch(inter.csr(), inter.row_of_edge(), 256, n, seed=SEED, step=step, n_neg=16, table=tab)
        got = ns.cpu().numpy()
        assert got.min() >= 0 and got.max() < n                    # n_items itself is never returned
        assert set(np.unique(got).tolist()) <= allowed             # nor a leading, inner or trailing zero-weight item
        seen |= set(np.unique(got).tolist())
        wu, wp, wn = E.sample(rowptr, col, 256, 16, E.cum_u32(tab), SEED, step)
        assert np.array_equal(us.cpu().numpy(), wu) and np.array_equal(ps.cpu().numpy(), wp) and np.array_equal(got, wn)
    assert seen == allowed                                          # both ends of the table are hit


# ---------------------------------------------------------------------------- 6: loss vs the float64 twin
def _small_batch(B, M, D, seed, U=5, I=6):
    """B slots on 11 nodes (tests/test_gpu_objectives.py): every row's references cross several 64-reference chunks."""
    g = t.Generator().manual_seed(seed)
    final = t.randn(U + I, D, generator=g) * (0.3 if D <= 128 else 0.09)
    e0 = t.randn(U + I, D, generator=g)
    users, pos = t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g)
    neg = t.randint(0, I, (B, M), generator=g)
    logq = t.linspace(-12.0, -1.0, I)[t.randperm(I, generator=g)].contiguous()
    return U, I, final, e0, users, pos, neg, logq


def _twin64(U, final, e0, users, pos, neg, lam, logq):
    f = final.double().requires_grad_(True)
    e = e0.double().requires_grad_(True)
    lq = logq.double()
    loss = E.twin_softmax_logq(f[users], e[users], f[U + pos], e[U + pos], f[U + neg], e[U + neg], lam, lq[pos], lq[neg])
    loss.backward()
    return loss.detach(), f.grad, e.grad


def _device_loss(ops, U, I, final, e0, users, pos, neg, lam, logq, with_map, objective="softmax"):
    """(loss, dense g_final [U + I, D], reg_w) of ops.rank_loss_fwd_bwd, through a node map or not."""
    B, M, D = users.numel(), neg.shape[1], final.shape[1]
    ud, pd, nd = users.to(DEV), pos.to(DEV), neg.to(DEV)
    lq = logq.to(DEV) if logq is not None else None
    reg_w = t.zeros(U + I, device=DEV)
    gf = t.zeros(U + I, D, device=DEV)
    if with_map:
        gmap, nodes, cnt = ops.batch_nodes(ud, pd, nd, U, U + I)
        c = int(cnt[0])
        rows = nodes[:c].long()
        compact = t.zeros((2 + M) * B, D, device=DEV)
        compact[:c] = final.to(DEV)[rows]
        gc = t.zeros((2 + M) * B, D, device=DEV)
        loss = ops.rank_loss_fwd_bwd(ud, pd, nd, compact, e0.to(DEV), U, lam, objective=objective, g_final=gc,
                                     reg_w=reg_w, node_map=gmap, logq=lq)
        gf[rows] = gc[:c]
        assert float(gc[c:].abs().max()) == 0.0
    else:
        loss = ops.rank_loss_fwd_bwd(ud, pd, nd, final.to(DEV), e0.to(DEV), U, lam, objective=objective, g_final=gf,
                                     reg_w=reg_w, logq=lq)
    return loss, gf, reg_w


@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("D", [4, 64, 512])
@pytest.mark.parametrize("M", [1, 4, 16])
def test_corrected_softmax_matches_float64_twin(M, D, with_map):
    ops = _ops()
    B, lam = 64, 1e-2
    U, I, final, e0, users, pos, neg, logq = _small_batch(B, M, D, seed=100 * M + D)
    want, g_fin, g_e0 = _twin64(U, final, e0, users, pos, neg, lam, logq)
    loss, gf, reg_w = _device_loss(ops, U, I, final, e0, users, pos, neg, lam, logq, with_map)
    plain = _device_loss(ops, U, I, final, e0, users, pos, neg, lam, None, with_map)
    print(f"M={M} D={D} map={with_map}: loss {float(loss):.9f} want {float(want):.9f} uncorrected {float(plain[0]):.9f} "
          f"max |dg| {float((gf.cpu().double() - g_fin).abs().max()):.3e}")
    assert _loss_close(loss, want)
    assert t.allclose(gf.cpu().double(), g_fin, atol=1e-6, rtol=1e-4)
    assert t.allclose((reg_w[:, None].cpu() * e0).double(), g_e0, atol=1e-6, rtol=1e-4)
    assert abs(float(loss) - float(plain[0])) > 1e-3               # the correction is not a no-op on this batch
    again = _device_loss(ops, U, I, final, e0, users, pos, neg, lam, logq, with_map)
    assert t.equal(loss, again[0]) and t.equal(gf, again[1]) and t.equal(reg_w, again[2])
    # a constant logq shifts every logit alike: the softmax does not move
    flat = _device_loss(ops, U, I, final, e0, users, pos, neg, lam, t.full((I,), -7.25), with_map)
    assert _loss_close(flat[0], plain[0])
    assert t.allclose(flat[1], plain[1], atol=1e-6, rtol=1e-4) and t.equal(flat[2], plain[2])


def _lq_entry(ops, objective, users, pos, neg, final, e0, n_users, lam, logq, g_scale):
    """mi_rank_loss_fwd_bwd_lq_f32 called directly, so that logq == NULL reaches the new entry."""
    from laplace_amd import _lib
    L = _lib.lib()
    B, M, D = users.numel(), neg.shape[1], final.shape[1]
    gf, rw, loss = t.zeros_like(final), t.zeros(final.shape[0], device=DEV), t.zeros(1, device=DEV)
    ws = t.empty(L.mi_rank_loss_workspace_bytes(B, M), dtype=t.uint8, device=DEV)
    rc = L.mi_rank_loss_fwd_bwd_lq_f32(B, M, _lib.MI_RANK_OBJECTIVES[objective], D, n_users, users.data_ptr(), pos.data_ptr(),
                                       neg.data_ptr(), final.data_ptr(), D, e0.data_ptr(), D, lam, g_scale, 1.0,
                                       loss.data_ptr(), gf.data_ptr(), D, rw.data_ptr(), None,
                                       logq.data_ptr() if logq is not None else None, ws.data_ptr(), ws.numel(),
                                       _lib.current_stream())
    t.cuda.synchronize()
    return rc, loss, gf, rw


@pytest.mark.parametrize("D", [4, 64, 100, 512])
@pytest.mark.parametrize("objective", ["reference", "bpr", "softmax"])
def test_null_logq_through_the_new_entry_is_bitwise_the_old_entry(objective, D):
    ops = _ops()
    lam = 1e-3
    U, I, final, e0, users, pos, neg, logq = _small_batch(300, 5, D, seed=D, U=40, I=25)
    ud, pd, nd, fd, ed = users.to(DEV), pos.to(DEV), neg.to(DEV), final.to(DEV), e0.to(DEV)
    ga, ra = t.zeros_like(fd), t.zeros(U + I, device=DEV)
    la = ops.rank_loss_fwd_bwd(ud, pd, nd, fd, ed, U, lam, objective=objective, g_final=ga, reg_w=ra, g_scale=1.0 / 3)
    rc, lb, gb, rb = _lq_entry(ops, objective, ud, pd, nd, fd, ed, U, lam, None, 1.0 / 3)
    assert rc == 0 and t.equal(la, lb) and t.equal(ga, gb) and t.equal(ra, rb)
    assert float(ga.abs().max()) > 0.0
    # a logq: the corrected softmax, and MI_ERR_UNSUPPORTED with nothing written for the other two
    rc, lc, gc, rw = _lq_entry(ops, objective, ud, pd, nd, fd, ed, U, lam, logq.to(DEV), 1.0 / 3)
    if objective == "softmax":
        assert rc == 0 and not t.equal(lc, la)
    else:
        from laplace_amd import _lib
        assert rc == _lib.MI_ERR_UNSUPPORTED and float(gc.abs().max()) == 0.0 and float(lc) == 0.0
        with pytest.raises(ValueError):
            ops.rank_loss_fwd_bwd(ud, pd, nd, fd, ed, U, lam, objective=objective, g_final=ga, logq=logq.to(DEV))
    for bad in (logq[:-1].to(DEV), logq.double().to(DEV), logq):   # a short table, another dtype, a CPU tensor
        with pytest.raises(Exception):
            ops.rank_loss_fwd_bwd(ud, pd, nd, fd, ed, U, lam, objective="softmax", g_final=ga, logq=bad)


def test_ranking_loss_autograd_function_with_logq():
    from laplace_amd.utils.metrics_lightgcn import ranking_loss
    g = t.Generator().manual_seed(4)
    B, M, D, lam = 48, 4, 64, 1e-3
    blocks = [t.randn(B, D, generator=g) * 0.4 for _ in range(4)] + [t.randn(B, M, D, generator=g) * 0.4 for _ in range(2)]
    pos_lq, neg_lq = -1.0 - 11.0 * t.rand(B, generator=g), -1.0 - 11.0 * t.rand(B, M, generator=g)
    dev = [x.to(DEV).requires_grad_(True) for x in blocks]
    ref = [x.double().requires_grad_(True) for x in blocks]
    loss = ranking_loss(*dev, lam, objective="softmax", logq=(pos_lq.to(DEV), neg_lq.to(DEV)))
    (2.0 * loss).backward()
    want = E.twin_softmax_logq(*ref, lam, pos_lq.double(), neg_lq.double())
    (2.0 * want).backward()
    assert _loss_close(loss, want)
    for a, b in zip(dev, ref):
        assert t.allclose(a.grad.cpu().double(), b.grad, atol=1e-6, rtol=1e-4)
    # [B, D] negatives with [B] logq; None is the function as it was
    two_d = [x.to(DEV) for x in blocks[:4]] + [blocks[4][:, 0].contiguous().to(DEV), blocks[5][:, 0].contiguous().to(DEV)]
    one = ranking_loss(*two_d, lam, objective="softmax", logq=(pos_lq.to(DEV), neg_lq[:, 0].contiguous().to(DEV)))
    want1 = E.twin_softmax_logq(*[x.double() for x in blocks[:4]], blocks[4][:, :1].double(), blocks[5][:, :1].double(), lam,
                                pos_lq.double(), neg_lq[:, :1].double())
    assert _loss_close(one, want1)
    assert t.equal(ranking_loss(*two_d, lam, objective="softmax", logq=None), ranking_loss(*two_d, lam, objective="softmax"))
    with pytest.raises(ValueError):
        ranking_loss(*two_d, lam, objective="bpr", logq=(pos_lq.to(DEV), neg_lq[:, 0].contiguous().to(DEV)))


# ---------------------------------------------------------------------------- 7: trainer
def _model_and_graph(U, I, n_edges, D, K, seed, compat):
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    g = t.Generator().manual_seed(seed)
    ei = t.stack([t.randint(0, U, (n_edges,), generator=g), t.randint(0, I, (n_edges,), generator=g)])
    t.manual_seed(seed)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K)
    inter = Interactions(ei, U, I)
    return model, inter, inter.adjacency(compat), ei


def test_trainer_ten_popularity_steps_match_autograd_loop():
    from laplace_amd.trainer import LightGCNTrainer
    U, I, n_edges, D, K, B, M, lam = 400, 600, 8000, 64, 3, 128, 4, 1e-6
    model, inter, adj, ei = _model_and_graph(U, I, n_edges, D, K, seed=21, compat="bipartite")
    uw = t.nn.Parameter(model.users_emb.weight.detach().clone())
    iw = t.nn.Parameter(model.items_emb.weight.detach().clone())
    opt = t.optim.Adam([uw, iw], lr=1e-3)
    row, col, _ = adj.coo()
    model.to(DEV)
    tr = LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), lr=1e-3, Lambda=lam, batch_size=B, seed=5,
                         objective="softmax", n_neg=M, negatives="popularity")
    assert tr.logq_correction and tr.neg_table is not None and tr.neg_table.power == 0.75 and tr.order is None
    degree = t.bincount(tr.train.csr().col.long().cpu(), minlength=I)
    q = np.diff(E.cum_u32(tr.neg_table).astype(np.int64), prepend=0)
    assert ((q == 0) == (degree.numpy() == 0)).all()
    logq = tr.neg_table.logq.cpu()
    drawn = []
    for it in range(10):
        ui, pi, ni = (x.cpu().clone() for x in tr.sample())
        drawn.append(ni)
        uf, u0, itf, it0 = R.lightgcn_forward(uw, iw, row, col, K)
        want = E.twin_softmax_logq(uf[ui], u0[ui], itf[pi], it0[pi], itf[ni], it0[ni], lam, logq[pi], logq[ni])
        opt.zero_grad()
        want.backward()
        opt.step()
        loss = tr.step((ui.to(DEV), pi.to(DEV), ni.to(DEV)))
        print(f"popularity softmax M={M} step {it}: loss {float(loss):.9f} twin {float(want):.9f}")
        assert _loss_close(loss, want.detach()), it
    assert (model.users_emb.weight.detach().cpu() - uw.detach()).abs().max() <= 1e-4
    assert (model.items_emb.weight.detach().cpu() - iw.detach()).abs().max() <= 1e-4
    drawn = t.cat(drawn)
    assert tuple(drawn.shape) == (10 * B, M) and int((degree[drawn] == 0).sum()) == 0
    # the batches step() draws itself are sample()'s: one more step each way
    peek = tuple(x.clone() for x in tr.sample())
    tr.step()
    assert all(t.equal(a, b) for a, b in zip(peek, tr.batch_idx))


def _run(steps=6, batches=None, **kw):
    """`steps` steps on test_step_forms_agree_and_repeat_bitwise's graph; batches: original ids to train on."""
    from laplace_amd.trainer import LightGCNTrainer
    U, I, n_edges, D, B = 900, 500, 15000, 64, 512
    model, inter, adj, ei = _model_and_graph(U, I, n_edges, D, 3, seed=41, compat="bipartite")
    model.to(DEV)
    kw.setdefault("objective", "softmax")
    kw.setdefault("n_neg", 4)
    tr = LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), lr=1e-3, Lambda=1e-4, batch_size=B, seed=9, **kw)
    losses, used = [], []
    for i in range(steps):
        batch = batches[i] if batches is not None else tuple(x.clone() for x in tr.sample())
        used.append(batch)
        losses.append(float(tr.step(batch)))
    tr.finish()
    return losses, used, tr.table.clone(), tr


def test_popularity_step_forms_agree_and_repeat_bitwise():
    """The dense step, the sparse_batch step and the reordered trainer on the same explicit original-id batches: a logq
    looked up in the wrong id space would move the reordered losses by far more than 1e-6."""
    pop = dict(negatives="popularity")
    plain = _run(sparse_batch=False, reorder=False, **pop)
    fast = _run(sparse_batch=True, reorder=False, **pop)
    again = _run(sparse_batch=True, reorder=False, **pop)
    ordered = _run(sparse_batch=True, reorder=True, batches=plain[1], **pop)
    ordered_plain = _run(sparse_batch=False, reorder=True, batches=plain[1], **pop)
    ordered_again = _run(sparse_batch=True, reorder=True, batches=plain[1], **pop)
    for a, b in zip(plain[1], fast[1]):                             # the same batches from the device sampler
        assert all(t.equal(x, y) for x, y in zip(a, b))
    for name, other in (("sparse", fast), ("reorder", ordered), ("reorder plain", ordered_plain)):
        print(name, "max |dloss|", max(abs(a - b) for a, b in zip(plain[0], other[0])), "max |dtable|",
              float((plain[2] - other[2]).abs().max()))
    for other in (fast, ordered, ordered_plain):
        for a, b in zip(plain[0], other[0]):
            assert abs(a - b) <= 1e-6
        assert (plain[2] - other[2]).abs().max() <= 2e-6
    assert fast[0] == again[0] and t.equal(fast[2], again[2])
    assert ordered[0] == ordered_again[0] and t.equal(ordered[2], ordered_again[2])
    # the reordered trainer's table lives in training ids: logq[new id] is the plain trainer's logq[old id]
    tr_o, tr_p = ordered[3], plain[3]
    assert tr_o.order is not None
    assert t.equal(tr_o.neg_table.logq[tr_o.order.item_new_of_old], tr_p.neg_table.logq)
    assert not t.equal(tr_o.neg_table.logq, tr_p.neg_table.logq)
    # its own sampler speaks original ids: positives are edges, negatives are not
    us, ps, ns = (x.cpu() for x in tr_o.sample())
    ei = _model_and_graph(900, 500, 15000, 64, 3, seed=41, compat="bipartite")[3]
    assert bool(_held(ei, 500, us, ps[:, None]).all()) and not bool(_held(ei, 500, us, ns).any())
    # without the correction the same negatives give another loss; with uniform negatives it is a constant shift
    raw = _run(sparse_batch=True, reorder=False, batches=plain[1], negatives="popularity", logq_correction=False)
    assert max(abs(a - b) for a, b in zip(raw[0], fast[0])) > 1e-3
    uni = _run(steps=3, sparse_batch=True, reorder=False)
    uni_lq = _run(steps=3, sparse_batch=True, reorder=False, logq_correction=True)
    assert all(abs(a - b) <= 1e-5 for a, b in zip(uni[0], uni_lq[0]))


def test_uniform_negatives_spelled_out_is_the_step_as_it_was():
    for kw in (dict(), dict(objective="reference", n_neg=1)):
        a = _run(**kw)
        b = _run(negatives="uniform", neg_power=0.75, logq_correction=None, **kw)
        assert a[0] == b[0] and t.equal(a[2], b[2])
        assert b[3].neg_table is None and b[3].logq is None
        for x, y in zip(a[1], b[1]):
            assert all(t.equal(p, q) for p, q in zip(x, y))


def test_pipeline_passes_the_negatives_through(tmp_path):
    """run_pipeline_lightgcn.train under compat="reference" (whose negative range and sampler quirk the popularity sampler
    leaves out): the trainer it builds draws from the table, and the run ends with finite statistics."""
    from dataclasses import replace
    from laplace_amd.config import lightgcn_config
    from laplace_amd.run_pipeline_lightgcn import train
    from test_gpu_acceptance import _tastes_graph
    cfg = replace(lightgcn_config, epochs=30, k=12, hidden_layer_size=32, learning_rate=1e-3, save_model=False, batch_size=128,
                  num_iterations=2, eval_every=100, lr_decay_every=100, Lambda=1e-6, show_graph=False, num_recommendations=64)
    ei = t.from_numpy(_tastes_graph(300, 200, 1000, seed=42).T.copy())
    out = {}
    for negatives in ("uniform", "popularity"):
        t.manual_seed(42)
        stats = train(cfg, edge_index=ei, num_users=300, num_articles=200, compat="reference", device=DEV, seed=42,
                      verbose=False, save_dir=str(tmp_path / negatives), objective="softmax", n_neg=4, predictor="propagated",
                      negatives=negatives, neg_power=0.75)
        for v in (stats.loss, stats.recall_val, stats.recall_test, stats.precision_val, stats.precision_test):
            assert np.isfinite(v)
        out[negatives] = stats.loss
    assert out["popularity"] != out["uniform"]                     # the training loss carries -log q
    with pytest.raises(ValueError):
        train(cfg, edge_index=ei, num_users=300, num_articles=200, device=DEV, verbose=False, negatives="zipf")


# ---------------------------------------------------------------------------- 8: state that outlives a call
def _scenario(which):
    if which == "uniform_m4":
        losses, _, table, _ = _run(steps=3)
    elif which == "popularity_m4":
        losses, _, table, _ = _run(steps=3, negatives="popularity")
    else:
        losses, _, table, _ = _run(steps=3, negatives="popularity", n_neg=7, neg_power=1.0)
    return [t.tensor(losses), table.cpu()]


def test_popularity_steps_after_other_steps_equal_fresh_process_values(tmp_path):
    """A popularity step after a uniform step in one process, and another at a different n_neg and power, against each run
    alone in a fresh process (the pattern of test_second_calls_with_other_shapes_equal_fresh_process_values)."""
    names = ("popularity_m4", "popularity_m7")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    procs = {}
    for name in names:
        out = str(tmp_path / f"{name}.pt")
        procs[name] = (out, subprocess.Popen([sys.executable, os.path.abspath(__file__), name, out], env=env,
                                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    got = {name: _scenario(name) for name in ("uniform_m4",) + names}
    for name in names:
        out, proc = procs[name]
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-2000:]
        fresh = t.load(out)
        assert len(got[name]) == len(fresh)
        for i, (a, b) in enumerate(zip(got[name], fresh)):
            assert t.equal(a, b), (name, i)


if __name__ == "__main__":   # one scenario of test 8 in a process of its own
    t.save(_scenario(sys.argv[1]), sys.argv[2])
