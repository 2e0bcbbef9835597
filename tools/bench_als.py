"""Time of an iALS epoch (als.ImplicitALS: a user half-sweep, then an item half-sweep) on the planted C1-scale graph, C2 and C3
at d = 64 and 128: the median of 11 epochs after warm-up, HIP events around each half-sweep (Gram product + row solves), all in
one process.  For each half-sweep the achieved rate of 2 d^2 nnz + rows d^3 / 3 flop is set against the 157 TF/s f32 matrix
peak.  One dense C2 LightGCN step (d = 128, 3 layers, batch 16 384) is timed in the same process for scale.
    python3 tools/bench_als.py [--shapes planted,c2,c3] [--dims 64,128] [--epochs 11] [--warmup 2] [--no-lightgcn]
One JSON line per (shape, d); nothing here is compared with a target: there is no earlier implementation."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as t
from laplace_amd import synthetic as S
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions

PEAK_TF = 157.0
PLANTED = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
SHAPES = {"planted": PLANTED, "c2": S.C2, "c3": S.C3}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="planted,c2,c3")
ap.add_argument("--dims", default="64,128")
ap.add_argument("--epochs", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-lightgcn", action="store_true")
args = ap.parse_args()


def half_sweep_ms(model, side):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    failed = model.half_sweep(side)
    b.record()
    return a, b, failed


for name in args.shapes.split(","):
    spec = SHAPES[name]
    t0 = time.perf_counter()
    ei = S.generate(spec)
    gen_s = time.perf_counter() - t0
    inter = Interactions(ei.cuda(), spec.num_users, spec.num_items)
    nnz = inter.num_edges
    for d in [int(x) for x in args.dims.split(",")]:
        model = ImplicitALS(spec.num_users, spec.num_items, dim=d, alpha=1.0, reg=20.0, seed=0).cuda()
        model.bind(inter)
        for _ in range(args.warmup):
            model.half_sweep("users"), model.half_sweep("items")
        t.cuda.synchronize()
        events, failed = [], 0
        for _ in range(args.epochs):
            events.append((half_sweep_ms(model, "users"), half_sweep_ms(model, "items")))
        t.cuda.synchronize()
        out = {"shape": name, "users": spec.num_users, "items": spec.num_items, "nnz": nnz, "d": d, "epochs": args.epochs,
               "generate_s": round(gen_s, 1)}
        for k, (side, rows) in enumerate((("users", spec.num_users), ("items", spec.num_items))):
            ms = statistics.median(e[k][0].elapsed_time(e[k][1]) for e in events)
            failed += sum(int(e[k][2].item()) for e in events)
            flop = 2.0 * d * d * nnz + rows * d ** 3 / 3.0
            out[f"{side}_ms"] = round(ms, 3)
            out[f"{side}_tflops"] = round(flop / (ms * 1e-3) / 1e12, 3)
            out[f"{side}_of_peak"] = round(flop / (ms * 1e-3) / 1e12 / PEAK_TF, 4)
        out["epoch_ms"] = round(out["users_ms"] + out["items_ms"], 3)
        out["failed_rows"] = failed
        print(json.dumps(out), flush=True)
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
