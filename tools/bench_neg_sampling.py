"""Popularity-weighted negatives: what they cost and what they are worth (profiles/neg_sampling.md).

  cost   ms per training step at BASELINE configs[1] (C2: 1M users x 100K items, 10M edges, D = 128, K = 3, batch 16 384),
         objective softmax with 4 negatives, uniform against popularity negatives (with the logQ correction): one graph, one
         trainer per leg, the legs' steps INTERLEAVED in one process, events around every step.  One JSON line per leg.
  worth  the recipe of tests/test_gpu_objectives.py::test_bounded_objectives_beat_the_reference_objective_and_popularity
         (C1-scale planted graph, spec seed 5, D 64, K 2, batch 1024, lr 1e-2, lambda 1e-6, 200 steps, bench.map_at_12):
         softmax with 4 negatives trained three ways — uniform; popularity 0.75 with the correction; popularity 0.75
         without — at trainer seeds 7, 8, 9.  One JSON line per run.

    python3 tools/bench_neg_sampling.py cost [--steps 20] [--warmup 5] [--small]
    python3 tools/bench_neg_sampling.py worth [--steps 200] [--seeds 7,8,9]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch as t
from laplace_amd import ops, synthetic as S
from laplace_amd.interactions import Interactions
from laplace_amd.model.lightgcn import LightGCN
from laplace_amd.trainer import LightGCNTrainer

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("cost", "worth"))
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--n-neg", type=int, default=4)
ap.add_argument("--power", type=float, default=0.75)
ap.add_argument("--seeds", default="7,8,9")
ap.add_argument("--small", action="store_true", help="cost on a C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
DEV = "cuda"


def cost():
    steps = args.steps or 20
    spec = S.C1 if args.small else S.C2
    D, K = (64, 2) if args.small else (128, 3)
    inter = Interactions(S.generate(spec).to(DEV), spec.num_users, spec.num_items)
    adj = inter.adjacency("bipartite")
    legs = {}
    for name in ("uniform", "popularity"):
        t.manual_seed(1234)
        model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to(DEV)
        legs[name] = LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=args.batch, seed=7,
                                     objective="softmax", n_neg=args.n_neg, negatives=name, neg_power=args.power)
    for _ in range(args.warmup):
        for tr in legs.values():
            tr.step()
    marks = {name: [] for name in legs}
    for _ in range(steps):   # uniform, popularity, uniform, ...: both legs see the same machine
        for name, tr in legs.items():
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            tr.step()
            b.record()
            marks[name].append((a, b))
    t.cuda.synchronize()
    for name, tr in legs.items():
        per = sorted(a.elapsed_time(b) for a, b in marks[name])
        print(json.dumps({"mode": "cost", "negatives": name, "objective": "softmax", "n_neg": args.n_neg, "batch": args.batch,
                          "logq_correction": tr.logq_correction, "steps": steps,
                          "ms_per_step_median": round(per[len(per) // 2], 3), "ms_per_step_min": round(per[0], 3),
                          "ms_per_step_max": round(per[-1], 3), "ms_per_step_mean": round(sum(per) / len(per), 3),
                          "compact_rows_last_step": int(tr.n_nodes[0]) if tr.sparse_batch else None,
                          "compact_rows_capacity": (2 + args.n_neg) * args.batch, "loss": round(float(tr.loss), 5)}),
              flush=True)
        tr.finish()


def worth():
    import bench
    steps = args.steps or 200
    spec = S.SyntheticSpec(num_users=S.C1.num_users, num_items=S.C1.num_items, num_edges=S.C1.num_edges, seed=5,
                           communities=8, community_mix=0.85, deg_min=1, deg_max=S.C1.num_items // 2)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).to(DEV)
    inter = Interactions(ei.to(DEV), spec.num_users, spec.num_items)
    degree = t.bincount(inter.edge_index[1], minlength=spec.num_items)
    head = t.zeros(spec.num_items, dtype=t.bool, device=DEV)
    head[t.argsort(degree, descending=True, stable=True)[: max(1, spec.num_items // 100)]] = True
    variants = (("uniform", dict()), ("popularity, corrected", dict(negatives="popularity", neg_power=args.power)),
                ("popularity, uncorrected", dict(negatives="popularity", neg_power=args.power, logq_correction=False)))
    for seed in (int(s) for s in args.seeds.split(",")):
        for name, kw in variants:
            t.manual_seed(0)
            model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
            tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024, seed=seed,
                                 objective="softmax", n_neg=args.n_neg, **kw)
            assert tr.order is None   # the replay below reads the sampler's ids as item ids
            got = bench.map_at_12(model, tr, inter, held, steps)
            # the negatives the run drew: the sampler is a function of (seed, step)
            in_head = total = 0
            for step in range(steps):
                neg = ops.sample_bpr_batch(tr._r, tr._row_of_edge, tr.batch_size, tr.neg_range, seed, step, n_neg=args.n_neg,
                                           table=tr.neg_table)[2]
                in_head += int(head[neg].sum())
                total += neg.numel()
            print(json.dumps({"mode": "worth", "variant": name, "trainer_seed": seed, "steps": steps, "n_neg": args.n_neg,
                              "propagated_map_at_12": round(got["propagated_embeddings_map_at_12"], 4),
                              "layer0_map_at_12": round(got["value"], 4),
                              "popularity_predictor_map_at_12": round(got["popularity_predictor_map_at_12"], 4),
                              "final_loss": round(float(tr.loss), 4),
                              "share_of_negatives_in_top_1pct_items": round(in_head / total, 4),
                              "share_of_edges_in_top_1pct_items": round(float(degree[head].sum()) / float(degree.sum()), 4)}),
                  flush=True)


cost() if args.mode == "cost" else worth()
