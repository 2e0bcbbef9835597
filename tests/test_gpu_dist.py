"""GPU: the user-sharded trainer with the HIP kernels, two ranks sharing the one card (gloo for the exchanges,
as in bench.py's rehearsal switch): together they must reproduce the single-process reference loop on the union
graph.  tests/test_dist_cpu.py checks the same host logic on the CPU with an oracle-backed kernel provider; this
one runs the product's own kernels — row-sliced CSRs with split rows, x_map / addend_map / row_list launches,
the Adam epilogue on the user rows — under a process group."""
import os
import socket
import sys

import pytest
import torch as t
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U0, U1, I, D, K, B, STEPS = 2500, 1800, 150, 64, 3, 512, 4


def _shards():
    g = t.Generator().manual_seed(0)
    out = []
    for U, E in ((U0, 60_000), (U1, 45_000)):  # ~700 users per item: item rows are split rows (> 256 entries)
        keys = t.randperm(U * I, generator=g)[:E]
        out.append(t.stack([keys // I, keys % I]))
    return out


def _tables():
    g = t.Generator().manual_seed(1)
    return t.randn(U0, D, generator=g) * 0.1, t.randn(U1, D, generator=g) * 0.1, t.randn(I, D, generator=g) * 0.1


def _batches(step):
    g = t.Generator().manual_seed(100 + step)
    return [(t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g), t.randint(0, I, (B,), generator=g))
            for U in (U0, U1)]


def _worker(rank, world, port, ret, sparse_batch, reorder=False):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t.cuda.set_device(0)
    from laplace_amd.dist import ShardedLightGCNTrainer
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    ei = _shards()[rank]
    tu0, tu1, ti = _tables()
    U = (U0, U1)[rank]
    model = LightGCN(U, I, D, K)
    with t.no_grad():
        model.users_emb.weight.copy_((tu0, tu1)[rank])
        model.items_emb.weight.copy_(ti if rank == 0 else t.zeros_like(ti))  # the constructor's broadcast must fix rank 1
    model.to("cuda")
    tr = ShardedLightGCNTrainer(model, Interactions(ei.cuda(), U, I), lr=1e-2, Lambda=1e-4, batch_size=B, seed=3,
                                sparse_batch=sparse_batch, reorder=reorder)
    assert tr.a_items.plan.n_long_rows > 0
    losses = []
    for s in range(STEPS):
        losses.append(float(tr.step(tuple(x.cuda() for x in _batches(s)[rank]))))
    fin = tr.forward().clone()
    item_order = None
    if reorder:  # rows back under their original (local) ids; the replicated items must be numbered alike on both ranks
        fin = fin[tr.order.node_new_of_old()]
        item_order = tr.order.item_new_of_old.cpu()
        tr.finish()
    ret[rank] = {"table": tr.table.cpu(), "final": fin.cpu(), "losses": losses, "item_order": item_order}
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("sparse_batch,reorder", [(True, False), (False, False), (True, True)])
def test_two_ranks_on_one_gpu_equal_the_single_process_reference(sparse_batch, reorder):
    from oracle import lightgcn_ref as R
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret, sparse_batch, reorder), nprocs=2, join=True)
    if reorder:
        assert t.equal(ret[0]["item_order"], ret[1]["item_order"])
    e0, e1 = _shards()
    eu, ei = t.cat([e0[0], e1[0] + U0]), t.cat([e0[1], e1[1]])
    row, col = R.bipartite_edges(eu, ei, U0 + U1)
    tu0, tu1, ti = _tables()
    uw, iw = t.nn.Parameter(t.cat([tu0, tu1])), t.nn.Parameter(ti.clone())
    opt = t.optim.Adam([uw, iw], lr=1e-2)
    for s in range(STEPS):
        b0, b1 = _batches(s)
        R.train_step(uw, iw, opt, row, col, K, (t.cat([b0[0], b1[0] + U0]), t.cat([b0[1], b1[1]]), t.cat([b0[2], b1[2]])), 1e-4)
    wu, _, wi, _ = R.lightgcn_forward(uw.detach(), iw.detach(), row, col, K)
    r0, r1 = ret[0], ret[1]
    assert t.equal(r0["table"][U0:], r1["table"][U1:])  # item replicas stay bitwise identical across ranks
    tol = 5e-6
    assert (r0["table"][:U0] - uw.detach()[:U0]).abs().max() <= tol and (r1["table"][:U1] - uw.detach()[U0:]).abs().max() <= tol
    assert (r0["table"][U0:] - iw.detach()).abs().max() <= tol
    assert (r0["final"][:U0] - wu[:U0]).abs().max() <= tol and (r1["final"][:U1] - wu[U0:]).abs().max() <= tol
    assert (r0["final"][U0:] - wi).abs().max() <= tol and (r1["final"][U1:] - wi).abs().max() <= tol


def test_bench_c4_four_ranks_on_one_card_smoke():
    """`bench.py --gpus 4` (the default configuration: BASELINE configs[3], ONE graph sharded by user over the ranks, strong
    scaling) rehearsed on this one-GPU box: the parent starts four fresh worker processes BEFORE anything touches the GPU (no
    re-exec), the ranks share the card (LAPLACE_BENCH_ONE_GPU=1) and gloo carries the item-row exchanges.  A reduced graph
    (64 000 x 2 000 x 640 000 in 64 user blocks, global batch 4 096), so that the line's bookkeeping is what is checked:
    n_gpus, strong scaling, the global batch split four ways, the workload string.  Four ranks, not the eight the node run
    uses: a GPU box of this pool allows at most six processes on the card at once (world sizes 4 and 8 of the sharded trainer
    itself: tests/test_dist_world_sizes.py, gloo on the CPU)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LAPLACE_BENCH_BACKEND="gloo", LAPLACE_BENCH_ONE_GPU="1", LAPLACE_BENCH_DEADLINE_S="300")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--users", "64000", "--items", "2000",
                        "--edges", "640000", "--batch", "4096", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"],
                       env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "positive-edges/s" and d["value"] > 0 and d["backend"] == "gloo"
    w = d["config"]["workload"]
    assert "sharded by user over 4 GPU(s)" in w and "16000 users" in w and "global batch 4096" in w and "configs[3]" in w
    assert abs(d["value"] - 4096 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6      # whole-job edges / max-over-ranks time
    assert d["roofline"]["dense_launches_per_step"] > 0 and "cpu_baseline" not in d
