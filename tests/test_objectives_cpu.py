"""No GPU: argument checks of the ranking objectives (Python surface and C entries) and a world-size-2 gloo run of the
sharded trainer with objective="softmax", n_neg=3 against the single-process autograd twin on the union graph."""
import os
import sys

import pytest
import torch as t
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_ops  # noqa: E402
from test_dist_cpu import B, D, I, K, U0, U1, _free_port, _shards, _tables  # noqa: E402

STEPS, M, LAM = 4, 3, 1e-4


def twin_loss(uf, u0, pf, p0, nf, n0, lam, objective):
    sp = (uf * pf).sum(-1)
    sn = (uf[:, None, :] * nf).sum(-1)
    x = sp[:, None] - sn
    if objective == "reference":
        main = -F.softplus(x).mean()
    elif objective == "bpr":
        main = F.softplus(-x).mean()
    else:
        main = (t.logsumexp(t.cat([sp[:, None], sn], dim=1), dim=1) - sp).mean()
    return main + lam * (u0.pow(2).sum() + p0.pow(2).sum() + n0.pow(2).sum())


# ---------------------------------------------------------------------------- argument checks
def _tiny_model():
    from laplace_amd.model.lightgcn import LightGCN
    return LightGCN(4, 5, 8, 1)


@pytest.mark.parametrize("kw", [dict(objective="hinge"), dict(objective=None), dict(n_neg=0), dict(n_neg=17),
                                dict(n_neg=2.0), dict(n_neg=True)])
def test_trainers_refuse_unknown_objectives_and_ranges(kw):
    from laplace_amd.dist import ShardedLightGCNTrainer
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(ValueError):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **kw)
    with pytest.raises(ValueError):
        ShardedLightGCNTrainer(_tiny_model(), None, lr=1e-3, Lambda=1e-6, batch_size=4, ops_impl=cpu_ops, **kw)


def test_ops_refuse_unknown_objectives_and_ranges():
    from laplace_amd import ops
    from laplace_amd.utils.metrics_lightgcn import ranking_loss
    u, p = t.zeros(4, dtype=t.int64), t.zeros(4, dtype=t.int64)
    tab = t.zeros(9, 8)
    with pytest.raises(ValueError):
        ops.rank_loss_fwd_bwd(u, p, t.zeros(4, 2, dtype=t.int64), tab, tab, 4, 1e-6, objective="hinge")
    for bad in (t.zeros(4, 17, dtype=t.int64), t.zeros(4, 0, dtype=t.int64), t.zeros(4, 2, 2, dtype=t.int64),
                t.zeros(5, 2, dtype=t.int64)):
        with pytest.raises(ValueError):
            ops.rank_loss_fwd_bwd(u, p, bad, tab, tab, 4, 1e-6, objective="bpr")
    with pytest.raises(ValueError):
        ops.batch_nodes(u, p, t.zeros(4, 17, dtype=t.int64), 4, 9)
    for n_neg in (0, 17, -1, 1.5):
        with pytest.raises(ValueError):
            ops.sample_bpr_batch(None, None, 4, 5, 0, 0, n_neg=n_neg)
    blocks = [t.zeros(4, 8)] * 4
    with pytest.raises(ValueError):
        ranking_loss(*blocks, t.zeros(4, 17, 8), t.zeros(4, 17, 8), 1e-6, objective="bpr")
    with pytest.raises(ValueError):
        ranking_loss(*blocks, t.zeros(4, 2, 8), t.zeros(4, 2, 8), 1e-6, objective="warp")
    with pytest.raises(ValueError):
        from laplace_amd.run_pipeline_lightgcn import train
        train(edge_index=t.zeros(2, 3, dtype=t.int64), num_users=2, num_articles=2, device="cpu", verbose=False,
              predictor="final")
    # with everything in range the call reaches the device check: no CPU fallback
    from laplace_amd._lib import MiError
    with pytest.raises(MiError):
        ops.rank_loss_fwd_bwd(u, p, t.zeros(4, 2, dtype=t.int64), tab, tab, 4, 1e-6, objective="bpr")


def test_c_entries_return_unsupported_before_anything_else():
    from laplace_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, BAD_ARG = _lib.MI_ERR_UNSUPPORTED, -1

    def rank(n_neg, objective, d=64):
        return L.mi_rank_loss_fwd_bwd_f32(8, n_neg, objective, d, 4, None, None, None, None, d, None, d, 1e-6, 1.0, 1.0, None,
                                          None, d, None, None, None, 0, None)
    for n_neg, objective in ((0, 0), (17, 1), (-3, 2), (1, 3), (4, -1)):
        assert rank(n_neg, objective) == UNSUPPORTED
    for objective in _lib.MI_RANK_OBJECTIVES.values():
        assert rank(1, objective) == BAD_ARG and rank(16, objective) == BAD_ARG      # in range: the null pointers are next
    for n_neg in (0, 17):
        assert L.mi_sample_bpr_batch_ex(8, n_neg, 10, None, None, None, 5, 0, 0, 0, 0, None, None, None, None) == UNSUPPORTED
        assert L.mi_batch_nodes_ex_i32(8, n_neg, 4, 9, None, None, None, None, None, None, None, 0, None) == UNSUPPORTED
    assert L.mi_sample_bpr_batch_ex(8, 3, 10, None, None, None, 5, 0, 0, 0, 0, None, None, None, None) == BAD_ARG
    assert L.mi_batch_nodes_ex_i32(8, 3, 4, 9, None, None, None, None, None, None, None, 0, None) == BAD_ARG
    assert sorted(_lib.MI_RANK_OBJECTIVES.items(), key=lambda kv: kv[1]) == [("reference", 0), ("bpr", 1), ("softmax", 2)]
    # workspace: grows with M, and covers the one-negative entry's at M = 1
    w = [L.mi_rank_loss_workspace_bytes(4096, m) for m in (1, 2, 8, 16)]
    assert w == sorted(w) and len(set(w)) == 4 and w[0] >= L.mi_bpr_workspace_bytes(4096)
    assert L.mi_rank_loss_workspace_bytes(-5, 99) > 0


# ---------------------------------------------------------------------------- sharded trainer, two ranks, gloo
class Provider:
    """tests/cpu_ops.py plus the calls the ranking objectives add to the provider contract."""

    def __getattr__(self, name):
        return getattr(cpu_ops, name)

    @staticmethod
    def sample_bpr_batch(r, row_of_edge, batch, neg_range, seed, step, quirk=False, out=None, edges_in_order=False,
                         no_self_loops=False, n_neg=1):
        g = t.Generator().manual_seed(int(seed) * 1000 + int(step))
        u, p, _ = cpu_ops.sample_bpr_batch(r, row_of_edge, batch, neg_range, seed, step, quirk, None, edges_in_order,
                                           no_self_loops)
        n = t.randint(0, neg_range, (batch, n_neg), generator=g)   # host logic only: any ids of the right shape
        if out is not None:
            for dst, src in zip(out, (u, p, n)):
                dst.copy_(src)
            return out
        return u, p, n

    @staticmethod
    def batch_nodes(users, pos, neg, n_users, n_nodes, *, gmap=None, nodes=None, count=None, ws=None):
        uniq = t.unique(t.cat([users, n_users + pos, n_users + neg.reshape(-1)]))
        gmap = gmap if gmap is not None else t.empty(n_nodes, dtype=t.int32)
        nodes = nodes if nodes is not None else t.zeros(users.numel() + pos.numel() + neg.numel(), dtype=t.int32)
        count = count if count is not None else t.zeros(2, dtype=t.int32)
        gmap.fill_(-1)
        gmap[uniq] = t.arange(uniq.numel(), dtype=t.int32)
        nodes[: uniq.numel()] = uniq.to(t.int32)
        count[0] = uniq.numel()
        count[1] = int((uniq < n_users).sum())
        return gmap, nodes, count

    @staticmethod
    def rank_loss_fwd_bwd(users, pos, neg, final_emb, e0, n_users, lambda_val, *, objective="reference", g_final=None,
                          reg_w=None, g_scale=1.0, reg_scale=1.0, loss_out=None, node_map=None):
        Un = n_users
        neg2 = neg.reshape(users.numel(), -1)
        f = (lambda idx: node_map[idx].long()) if node_map is not None else (lambda idx: idx)
        rows = [final_emb[f(users)], e0[users], final_emb[f(Un + pos)], e0[Un + pos], final_emb[f(Un + neg2)], e0[Un + neg2]]
        rows = [x.detach().requires_grad_(True) for x in rows]
        loss = twin_loss(*rows, lambda_val, objective)
        if g_final is not None:
            grads = t.autograd.grad(loss, rows)
            d = final_emb.shape[1]
            for idx, gf in ((users, grads[0]), (Un + pos, grads[2]), (Un + neg2.reshape(-1), grads[4].reshape(-1, d))):
                g_final.index_add_(0, f(idx), g_scale * gf)
                if reg_w is not None:
                    reg_w.index_add_(0, idx, t.full((idx.numel(),), 2.0 * lambda_val * reg_scale))
        if loss_out is None:
            loss_out = t.empty(1)
        loss_out[0] = loss.detach()
        return loss_out


def _batches(step):
    g = t.Generator().manual_seed(200 + step)
    return [(t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g), t.randint(0, I, (B, M), generator=g))
            for U in (U0, U1)]


def _worker(rank, world, port, ret, sparse_batch, reorder):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import datetime
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t.set_num_threads(2)
    from laplace_amd.dist import ShardedLightGCNTrainer
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    ei = _shards()[rank]
    tu0, tu1, ti = _tables()
    U = (U0, U1)[rank]
    model = LightGCN(U, I, D, K)
    with t.no_grad():
        model.users_emb.weight.copy_((tu0, tu1)[rank])
        model.items_emb.weight.copy_(ti if rank == 0 else t.zeros_like(ti))
    tr = ShardedLightGCNTrainer(model, Interactions(ei, U, I), lr=1e-2, Lambda=LAM, batch_size=B, seed=3,
                                ops_impl=Provider(), sparse_batch=sparse_batch, reorder=reorder, objective="softmax",
                                n_neg=M)
    losses = [float(tr.step(_batches(s)[rank])) for s in range(STEPS)]
    b = _batches(0)[rank]
    try:   # a [B] negative against tables sized for M: refused, as LightGCNTrainer refuses it
        tr.step((b[0], b[1], b[2][:, 0].contiguous()))
        refused = False
    except ValueError:
        refused = True
    us, ps, ns = tr.sample()
    shapes = (tuple(us.shape), tuple(ps.shape), tuple(ns.shape), tr.nodes.numel() if sparse_batch else None)
    fin = tr.forward().clone()
    if reorder:
        fin = fin[tr.order.node_new_of_old()]
        tr.finish()
    ret[rank] = {"table": tr.table.clone(), "final": fin, "losses": losses, "shapes": shapes, "refused": refused}
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("sparse_batch,reorder", [(False, False), (True, False), (True, True)])
def test_two_rank_softmax_three_negatives_equals_single_process_twin(sparse_batch, reorder):
    from oracle import lightgcn_ref as R
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret, sparse_batch, reorder), nprocs=2, join=True)
    e0, e1 = _shards()
    eu, ei = t.cat([e0[0], e1[0] + U0]), t.cat([e0[1], e1[1]])
    row, col = R.bipartite_edges(eu, ei, U0 + U1)
    tu0, tu1, ti = _tables()
    uw, iw = t.nn.Parameter(t.cat([tu0, tu1])), t.nn.Parameter(ti.clone())
    opt = t.optim.Adam([uw, iw], lr=1e-2)
    for s in range(STEPS):
        b0, b1 = _batches(s)
        ui, pi, ni = t.cat([b0[0], b1[0] + U0]), t.cat([b0[1], b1[1]]), t.cat([b0[2], b1[2]])
        uf, u0_, itf, it0 = R.lightgcn_forward(uw, iw, row, col, K)
        loss = twin_loss(uf[ui], u0_[ui], itf[pi], it0[pi], itf[ni], it0[ni], LAM, "softmax")
        opt.zero_grad()
        loss.backward()
        opt.step()
    wu, _, wi, _ = R.lightgcn_forward(uw.detach(), iw.detach(), row, col, K)
    r0, r1 = ret[0], ret[1]
    assert t.equal(r0["table"][U0:], r1["table"][U1:])                     # item replicas: bitwise identical
    tol = 5e-6
    assert (r0["table"][:U0] - uw.detach()[:U0]).abs().max() <= tol and (r1["table"][:U1] - uw.detach()[U0:]).abs().max() <= tol
    assert (r0["table"][U0:] - iw.detach()).abs().max() <= tol
    assert (r0["final"][:U0] - wu[:U0]).abs().max() <= tol and (r1["final"][:U1] - wu[U0:]).abs().max() <= tol
    assert (r0["final"][U0:] - wi).abs().max() <= tol and (r1["final"][U1:] - wi).abs().max() <= tol
    assert all(0.0 < x < 10.0 for x in r0["losses"] + r1["losses"])       # log(1 + M) at the start, never negative
    for r in (r0, r1):
        assert r["refused"]
        assert r["shapes"][:3] == ((B,), (B,), (B, M)) and r["shapes"][3] in (None, (2 + M) * B)
