"""In-batch negatives: what they cost and what they are worth (profiles/inbatch_softmax.md).

  cost   ms per training step at BASELINE configs[1] (C2: 1M users x 100K items, 10M edges, D = 128, K = 3, batch 16 384),
         objective softmax: in-batch negatives at G = 256, 1024, 4096 against uniform negatives with 4 and with 16 drawn per
         positive.  One graph, one trainer per leg, the legs' steps INTERLEAVED in one process, events around every step.
         One JSON line per leg.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_inbatch.py cost ...` the
         same run gives the per-kernel times.
  worth  the recipe of profiles/neg_sampling.md section 4 (tools/bench_neg_sampling.py worth), unchanged: C1-scale planted
         graph, spec seed 5, D 64, K 2, batch 1024, lr 1e-2, lambda 1e-6, 200 steps, bench.map_at_12, trainer seeds 7, 8, 9.
         Legs: in-batch corrected at G = 256 and 1024, in-batch uncorrected at 1024, uniform softmax with 4 and with 16
         negatives.  One JSON line per run.

    python3 tools/bench_inbatch.py cost [--steps 20] [--warmup 5] [--small] [--legs "in_batch G=1024"]
    python3 tools/bench_inbatch.py worth [--steps 200] [--seeds 7,8,9]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch as t
from laplace_amd import synthetic as S
from laplace_amd.interactions import Interactions
from laplace_amd.model.lightgcn import LightGCN
from laplace_amd.trainer import LightGCNTrainer

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("cost", "worth"))
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--seeds", default="7,8,9")
ap.add_argument("--legs", default=None, help='cost: only the legs whose names are listed, e.g. "in_batch G=1024,uniform M=16"')
ap.add_argument("--small", action="store_true", help="cost on a C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
DEV = "cuda"


def cost():
    steps = args.steps or 20
    spec = S.C1 if args.small else S.C2
    D, K = (64, 2) if args.small else (128, 3)
    inter = Interactions(S.generate(spec).to(DEV), spec.num_users, spec.num_items)
    adj = inter.adjacency("bipartite")
    variants = [(f"in_batch G={g}", dict(negatives="in_batch", in_batch_group=g)) for g in (256, 1024, 4096)]
    variants += [(f"uniform M={m}", dict(n_neg=m)) for m in (4, 16)]
    if args.legs is not None:
        variants = [v for v in variants if v[0] in args.legs.split(",")]
    legs = {}
    for name, kw in variants:
        t.manual_seed(1234)
        model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to(DEV)
        legs[name] = LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=args.batch, seed=7,
                                     objective="softmax", **kw)
    for _ in range(args.warmup):
        for tr in legs.values():
            tr.step()
    marks = {name: [] for name in legs}
    for _ in range(steps):   # one step of every leg in turn: all legs see the same machine
        for name, tr in legs.items():
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            tr.step()
            b.record()
            marks[name].append((a, b))
    t.cuda.synchronize()
    for name, tr in legs.items():
        per = sorted(a.elapsed_time(b) for a, b in marks[name])
        print(json.dumps({"mode": "cost", "leg": name, "objective": "softmax", "batch": args.batch,
                          "logq_correction": tr.logq_correction, "steps": steps,
                          "ms_per_step_median": round(per[len(per) // 2], 3), "ms_per_step_min": round(per[0], 3),
                          "ms_per_step_max": round(per[-1], 3),
                          "unique_batch_rows_last_step": int(tr.n_nodes[0]) if tr.sparse_batch else None,
                          "batch_references": (2 if tr.in_batch else 2 + tr.n_neg) * args.batch,
                          "loss": round(float(tr.loss), 5)}), flush=True)
        tr.finish()


def worth():
    import bench
    steps = args.steps or 200
    spec = S.SyntheticSpec(num_users=S.C1.num_users, num_items=S.C1.num_items, num_edges=S.C1.num_edges, seed=5,
                           communities=8, community_mix=0.85, deg_min=1, deg_max=S.C1.num_items // 2)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).to(DEV)
    inter = Interactions(ei.to(DEV), spec.num_users, spec.num_items)
    variants = (("in_batch G=256, corrected", dict(negatives="in_batch", in_batch_group=256)),
                ("in_batch G=1024, corrected", dict(negatives="in_batch", in_batch_group=1024)),
                ("in_batch G=1024, uncorrected", dict(negatives="in_batch", in_batch_group=1024, logq_correction=False)),
                ("uniform M=4", dict(n_neg=4)), ("uniform M=16", dict(n_neg=16)))
    for seed in (int(s) for s in args.seeds.split(",")):
        for name, kw in variants:
            t.manual_seed(0)
            model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
            tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024, seed=seed,
                                 objective="softmax", **kw)
            got = bench.map_at_12(model, tr, inter, held, steps)
            print(json.dumps({"mode": "worth", "variant": name, "trainer_seed": seed, "steps": steps,
                              "propagated_map_at_12": round(got["propagated_embeddings_map_at_12"], 4),
                              "layer0_map_at_12": round(got["value"], 4),
                              "popularity_predictor_map_at_12": round(got["popularity_predictor_map_at_12"], 4),
                              "final_loss": round(float(tr.loss), 4)}), flush=True)


cost() if args.mode == "cost" else worth()
