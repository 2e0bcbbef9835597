"""Time of an iALS epoch (als.ImplicitALS: a user half-sweep, then an item half-sweep) on the planted C1-scale graph, C2 and C3
at d = 64 and 128: the median of 11 epochs after warm-up, HIP events around each half-sweep (Gram product + row solves), all in
one process.  For each half-sweep the achieved rate of 2 d^2 nnz + rows d^3 / 3 flop is set against the 157 TF/s f32 matrix
peak.  One dense C2 LightGCN step (d = 128, 3 layers, batch 16 384) is timed in the same process for scale.
    python3 tools/bench_als.py [--shapes planted,c2,c3] [--dims 64,128] [--epochs 11] [--warmup 2] [--no-lightgcn]
                               [--solver cholesky|block|both] [--block 16,32] [--sweeps 1,2] [--dim D] [--fold-in]
                               [--weighted] [--reg-power NU] [--hub-threshold none,256,1024,4096]
--solver block / both adds one line per (block, sweeps) with the block row solver (ops.als_block_rows) from the SAME initial
tables as the Cholesky line of that (shape, d) — the yardstick, timed in the same run; d > 128 has the block lines only.  A
block line also carries hub_ms: the one longest item row alone through row_list, i.e. the one wavefront the item
half-sweep cannot end before.  --dim D is --dims D.  --fold-in adds, per (shape, d, block), what a fold-in from zero leaves
after 1, 2, 4 and 8 sweeps on the first 4 096 users: the relative distance to the same rows after 64 sweeps.
--weighted adds, after every line, the same configuration from the same initial tables through the WEIGHTED entries: first
with a_e == alpha on every edge (weights "constant": the same operands as the unweighted line, so the ratio of the two is the
cost of the weighted kernels alone), then with a random weight per edge in [0.1, 30] / alpha and --reg-power NU (weights
"random").  Each weighted line carries users_vs_unweighted / items_vs_unweighted, its time over the unweighted line's.
--hub-threshold LIST repeats every block line per entry of the list: "none" is the block entry as it was (the yardstick, in the
same run), an integer T takes the rows with more than T entries through the hub entries (ops.als_block_rows(hub_threshold=T)).
Such a line carries hub_threshold, the hub rows and chunks of both sides, the larger of the two workspaces in bytes, and its
hub_ms is the longest item row alone through row_list WITH that threshold.
One JSON line per (shape, d, solver); the flop model of every line is the full solve's, so TF/s of a block line is a
speed-up in disguise, not a rate."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as t
from laplace_amd import ops, synthetic as S
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions

PEAK_TF = 157.0
PLANTED = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
SHAPES = {"planted": PLANTED, "c2": S.C2, "c3": S.C3}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="planted,c2,c3")
ap.add_argument("--dims", default="64,128")
ap.add_argument("--dim", type=int, default=None)
ap.add_argument("--epochs", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-lightgcn", action="store_true")
ap.add_argument("--solver", default="cholesky", choices=["cholesky", "block", "both"])
ap.add_argument("--block", default="16")
ap.add_argument("--sweeps", default="1")
ap.add_argument("--fold-in", action="store_true")
ap.add_argument("--weighted", action="store_true")
ap.add_argument("--reg-power", type=float, default=0.5)
ap.add_argument("--hub-threshold", default="none")
args = ap.parse_args()
dims = [args.dim] if args.dim is not None else [int(x) for x in args.dims.split(",")]
hub_thresholds = [None if x.strip().lower() == "none" else int(x) for x in args.hub_threshold.split(",")]
block_cfgs = [(int(b), int(s), h) for b in args.block.split(",") for s in args.sweeps.split(",") for h in hub_thresholds]


def half_sweep_ms(model, side):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    failed = model.half_sweep(side)
    b.record()
    return a, b, failed


def timed(fn, reps):
    fn()
    t.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        t.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


for name in args.shapes.split(","):
    spec = SHAPES[name]
    t0 = time.perf_counter()
    ei = S.generate(spec)
    gen_s = time.perf_counter() - t0
    inter = Interactions(ei.cuda(), spec.num_users, spec.num_items)
    nnz = inter.num_edges
    for d in dims:
        cfgs = [("cholesky", 16, 1, None)] if args.solver != "block" and d <= ops.ALS_MAX_DIM else []
        if args.solver != "cholesky":
            cfgs += [("block", b, s, h) for b, s, h in block_cfgs]
        model = ImplicitALS(spec.num_users, spec.num_items, dim=d, alpha=1.0, reg=20.0, seed=0, solver="block").cuda()
        model.bind(inter)
        start = (model.users_emb.weight.clone(), model.items_emb.weight.clone())
        base = {}
        modes = [("none", None, 0.0)]
        if args.weighted:
            gen = t.Generator(device="cuda").manual_seed(1)
            lo, hi = t.log(t.tensor(0.1)).item(), t.log(t.tensor(30.0)).item()
            w_rand = t.exp(t.rand(nnz, generator=gen, device="cuda", dtype=t.float64) * (hi - lo) + lo) / model.alpha
            modes += [("constant", t.ones(nnz, dtype=t.float32, device="cuda"), 0.0), ("random", w_rand, args.reg_power)]
        for (solver, block, sweeps, hub_thr), (weights, conf, nu) in ((c, m) for c in cfgs for m in modes):
            model.solver, model.block, model.block_sweeps, model.hub_threshold = solver, block, sweeps, hub_thr
            model.reg_power = nu
            model.reg = 20.0 if nu == 0.0 else 20.0 / (spec.num_items + nnz / spec.num_users) ** nu   # about 20 on a mean user row
            model.bind(inter, conf)
            model.users_emb.weight.copy_(start[0])
            model.items_emb.weight.copy_(start[1])
            for _ in range(args.warmup):
                model.half_sweep("users"), model.half_sweep("items")
            t.cuda.synchronize()
            events, failed = [], 0
            for _ in range(args.epochs):
                events.append((half_sweep_ms(model, "users"), half_sweep_ms(model, "items")))
            t.cuda.synchronize()
            out = {"shape": name, "users": spec.num_users, "items": spec.num_items, "nnz": nnz, "d": d, "solver": solver,
                   "epochs": args.epochs, "generate_s": round(gen_s, 1)}
            if solver == "block":
                out.update(block=block, sweeps=sweeps, hub_threshold=hub_thr)
                if hub_thr is not None:
                    L, ws = ops._lib.lib(), 0
                    for side, k in (("users", 1), ("items", 2)):
                        csr = model._bound[k]
                        hr, hc = ops.als_hub_counts(csr, hub_thr, d)
                        out[f"{side}_hub_rows"], out[f"{side}_hub_chunks"] = hr, hc
                        ws = max(ws, int(L.mi_als_block_rows_hub_workspace_bytes(csr.n_rows, csr.nnz, d, block, hr, hc)))
                    out["hub_workspace_bytes"] = ws
            if args.weighted:
                out.update(weights=weights, reg_power=nu)
            for k, (side, rows) in enumerate((("users", spec.num_users), ("items", spec.num_items))):
                ms = statistics.median(e[k][0].elapsed_time(e[k][1]) for e in events)
                failed += sum(int(e[k][2].item()) for e in events)
                flop = 2.0 * d * d * nnz + rows * d ** 3 / 3.0
                out[f"{side}_ms"] = round(ms, 3)
                out[f"{side}_tflops"] = round(flop / (ms * 1e-3) / 1e12, 3)
                out[f"{side}_of_peak"] = round(flop / (ms * 1e-3) / 1e12 / PEAK_TF, 4)
            out["epoch_ms"] = round(out["users_ms"] + out["items_ms"], 3)
            if weights == "none":
                base = {side: out[f"{side}_ms"] for side in ("users", "items")}
            else:
                for side in ("users", "items"):
                    out[f"{side}_vs_unweighted"] = round(out[f"{side}_ms"] / base[side], 3)
            out["failed_rows"] = failed
            out["objective"] = round(model.objective(inter), 2) if name == "planted" else None
            if solver == "block" and weights == "none":
                by_item = model._bound[2]
                deg = by_item.rowptr[1:] - by_item.rowptr[:-1]
                hub = deg.argmax().to(t.int32).reshape(1)
                X, G = model.users_emb.weight.data, ops.gemm(model.users_emb.weight.data, model.users_emb.weight.data,
                                                             trans_a=True, trans_b=False)
                x1 = model.items_emb.weight.data[hub.long()].clone()
                out["hub_entries"] = int(deg.max().item())
                out["hub_ms"] = round(timed(lambda: ops.als_block_rows(by_item, X, G, alpha=1.0, reg=20.0, block=block,
                                                                       sweeps=sweeps, x=x1, row_list=hub,
                                                                       hub_threshold=hub_thr), 5), 3)
            print(json.dumps(out), flush=True)
            if solver == "block" and weights == "none" and args.fold_in and sweeps == block_cfgs[0][1] and hub_thr is None:
                by_user = model._bound[1]
                rl = t.arange(min(4096, spec.num_users), dtype=t.int32, device="cuda")
                Y = model.items_emb.weight.data
                G = ops.gemm(Y, Y, trans_a=True, trans_b=False)
                ref = ops.als_block_rows(by_user, Y, G, alpha=1.0, reg=20.0, block=block, sweeps=64, row_list=rl)[0]
                left = {}
                for s in (1, 2, 4, 8):
                    x = ops.als_block_rows(by_user, Y, G, alpha=1.0, reg=20.0, block=block, sweeps=s, row_list=rl)[0]
                    rel = (x - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)
                    left[str(s)] = {"median": float(rel.median()), "max": float(rel.max())}
                print(json.dumps({"shape": name, "d": d, "block": block, "fold_in_relative_distance_to_64_sweeps": left}), flush=True)
        del model
    del inter
    t.cuda.empty_cache()

if not args.no_lightgcn:
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    spec = S.C2
    inter = Interactions(S.generate(spec).cuda(), spec.num_users, spec.num_items)
    t.manual_seed(1234)
    model = LightGCN(spec.num_users, spec.num_items, embedding_dim=128, num_iterations=3).cuda()
    tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-3, Lambda=1e-6, batch_size=16384, seed=7,
                         sparse_batch=False)
    for _ in range(3):
        tr.step()
    t.cuda.synchronize()
    ms = []
    for _ in range(11):
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        tr.step()
        b.record()
        t.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    tr.finish()
    print(json.dumps({"shape": "c2", "lightgcn_dense_step_ms": round(statistics.median(ms), 3), "d": 128, "layers": 3,
                      "batch": 16384}), flush=True)
