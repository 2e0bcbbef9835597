"""ms per training step at BASELINE configs[1] (C2: 1M users x 100K items, 10M edges, D = 128, K = 3, batch 16 384)
for the ranking objectives: (reference, 1) — the default step — against (bpr, 1), (bpr, 4), (softmax, 4), ...
One graph, one trainer per leg, events around --steps steps after --warmup.  Prints one JSON line per leg.
    python3 tools/bench_objectives.py [--legs reference:1,bpr:1,bpr:4,softmax:4] [--steps 20] [--warmup 5] [--small]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as t
from laplace_amd import synthetic as S
from laplace_amd.interactions import Interactions
from laplace_amd.model.lightgcn import LightGCN
from laplace_amd.trainer import LightGCNTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="reference:1,bpr:1,bpr:4,softmax:4")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--small", action="store_true", help="C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
spec = S.C1 if args.small else S.C2
D, K = (64, 2) if args.small else (128, 3)
inter = Interactions(S.generate(spec).to("cuda"), spec.num_users, spec.num_items)
adj = inter.adjacency("bipartite")
for leg in args.legs.split(","):
    objective, m = leg.split(":")
    t.manual_seed(1234)
    model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to("cuda")
    tr = LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=args.batch, seed=7, objective=objective,
                         n_neg=int(m))
    for _ in range(args.warmup):
        tr.step()
    marks = [t.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    marks[0].record()
    for i in range(args.steps):
        tr.step()
        marks[i + 1].record()
    t.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    rows = int(tr.n_nodes[0]) if tr.sparse_batch else None
    print(json.dumps({"objective": objective, "n_neg": int(m), "batch": args.batch, "ms_per_step_mean": round(sum(per) / len(per), 3),
                      "ms_per_step_median": round(per[len(per) // 2], 3), "ms_per_step_min": round(per[0], 3),
                      "compact_rows_last_step": rows, "compact_rows_capacity": (2 + int(m)) * args.batch,
                      "loss": round(float(tr.loss), 5)}), flush=True)
    tr.finish()
    del tr, model
