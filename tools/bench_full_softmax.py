#!/usr/bin/env python3
"""The exact full-catalogue softmax: what it costs and what it is worth (profiles/full_softmax.md).

  kernel  ops.full_softmax_fwd_bwd at B = 16 384, I = 100 000, d in --dims (64, 128): median of 11 calls after a warm-up, device
          events around each call, ms and TF/s of 10 B I d flops (three score products and two gradient products) against the
          f32 matrix peak.  Yardstick, in the same run and in turn with it: ops.rank_of_items on the same operands (one
          score product with integer compares); the expectation to judge against is 5 x that time x 1.5.  The loss-only
          form is timed too: one score product plus the exponentials.
  cost    ms per training step at C2 (1M users x 100K items, 10M edges, D = 128, K = 3, batch 16 384), sparse_batch=False,
          objective softmax: full_softmax=True against the same dense step with 1 and with 16 drawn negatives.  One trainer per
          leg, the legs' steps INTERLEAVED in one process, events around every step; three runs per leg (--runs).
  worth   the recipe of profiles/neg_sampling.md section 4: C1-scale planted graph, spec seed 5, D 64, K 2, batch 1024, lr 1e-2,
          lambda 1e-6, 200 steps, bench.map_at_12, trainer seeds 7, 8, 9.  Legs: uniform with 4 and with 16 negatives, in-batch
          at G = 1024 corrected, the full softmax.  Propagated MAP@12 and full_rank_metrics of the propagated tables on the
          held-out edges (recall@100, MRR, AUC).
  all     the three modes as child processes, each under its own time limit, stopping at the first that does not end well.
One JSON line per leg.

    python3 tools/bench_full_softmax.py kernel [--rows 16384] [--items 100000] [--dims 64,128] [--reps 11]
    python3 tools/bench_full_softmax.py cost [--steps 10] [--warmup 3] [--runs 3] [--small]
    python3 tools/bench_full_softmax.py worth [--steps 200] [--seeds 7,8,9]
    python3 tools/bench_full_softmax.py all"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 MFMA (the figure profiles/inbatch_softmax.md uses)
LIMITS = {"kernel": 300, "cost": 900, "worth": 600}   # seconds a mode may take as a child of `all`

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("kernel", "cost", "worth", "all"))
ap.add_argument("--rows", type=int, default=16384)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--dims", default="64,128")
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--seeds", default="7,8,9")
ap.add_argument("--small", action="store_true", help="cost on a C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
DEV = "cuda"


def kernel():
    import torch as t
    from laplace_amd import ops
    B, I, reps = args.rows, args.items, args.reps
    g = t.Generator(device=DEV).manual_seed(0)
    for d in (int(x) for x in args.dims.split(",")):
        final = t.randn(B + I, d, device=DEV, generator=g) * 0.1          # B user rows (one per slot), then the catalogue
        users = t.arange(B, device=DEV)
        pos = t.randint(0, I, (B,), device=DEV, generator=g)
        gf, rw, out = t.zeros(B + I, d, device=DEV), t.zeros(B + I, device=DEV), t.zeros(1, device=DEV)
        ue, ie = final[:B], final[B:]
        legs = {"full_softmax_fwd_bwd": lambda: ops.full_softmax_fwd_bwd(users, pos, final, final, B, 1e-6, g_final=gf, reg_w=rw,
                                                                         loss_out=out),
                "full_softmax_fwd_bwd, loss only": lambda: ops.full_softmax_fwd_bwd(users, pos, final, final, B, 1e-6, loss_out=out),
                "rank_of_items": lambda: ops.rank_of_items(users, pos, ue, ie)}
        ms = {name: [] for name in legs}
        for rep in range(reps + 2):          # two warm-up rounds; the legs take turns inside every repetition
            for name, fn in legs.items():
                a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 2:
                    ms[name].append(a.elapsed_time(b))
        med = {name: statistics.median(v) for name, v in ms.items()}
        flops = {"full_softmax_fwd_bwd": 10.0, "full_softmax_fwd_bwd, loss only": 2.0, "rank_of_items": 2.0}
        for name, v in ms.items():
            f = flops[name] * B * I * d
            print(json.dumps({"mode": "kernel", "leg": name, "rows": B, "items": I, "d": d, "ms_median": round(med[name], 4),
                              "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "reps": len(v),
                              "flops": f, "tflops": round(f / (med[name] * 1e-3) / 1e12, 2),
                              "share_of_f32_matrix_peak": round(f / (med[name] * 1e-3) / F32_MATRIX_PEAK, 4),
                              "ratio_to_rank_of_items": round(med[name] / med["rank_of_items"], 3),
                              "expectation_ratio": 7.5, "loss": round(float(out), 6)}), flush=True)


def cost():
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    steps = args.steps or 10
    spec = S.C1 if args.small else S.C2
    D, K = (64, 2) if args.small else (128, 3)
    inter = Interactions(S.generate(spec).to(DEV), spec.num_users, spec.num_items)
    adj = inter.adjacency("bipartite")
    variants = (("full softmax", dict(full_softmax=True)), ("uniform M=1", dict(n_neg=1)), ("uniform M=16", dict(n_neg=16)))
    legs = {}
    for name, kw in variants:
        t.manual_seed(1234)
        model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to(DEV)
        legs[name] = LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=args.batch, seed=7,
                                     objective="softmax", sparse_batch=False, **kw)
    for _ in range(args.warmup):
        for tr in legs.values():
            tr.step()
    for run in range(args.runs):
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
            print(json.dumps({"mode": "cost", "run": run, "leg": name, "objective": "softmax", "sparse_batch": False,
                              "batch": args.batch, "steps": steps, "ms_per_step_median": round(per[len(per) // 2], 3),
                              "ms_per_step_min": round(per[0], 3), "ms_per_step_max": round(per[-1], 3),
                              "loss": round(float(tr.loss), 5)}), flush=True)


def worth():
    import torch as t
    import bench
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn
    steps = args.steps or 200
    spec = S.SyntheticSpec(num_users=S.C1.num_users, num_items=S.C1.num_items, num_edges=S.C1.num_edges, seed=5,
                           communities=8, community_mix=0.85, deg_min=1, deg_max=S.C1.num_items // 2)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).to(DEV)
    inter = Interactions(ei.to(DEV), spec.num_users, spec.num_items)
    variants = (("uniform M=4", dict(n_neg=4)), ("uniform M=16", dict(n_neg=16)),
                ("in_batch G=1024, corrected", dict(negatives="in_batch", in_batch_group=1024)),
                ("full softmax", dict(full_softmax=True, sparse_batch=False)))
    U = spec.num_users
    for seed in (int(s) for s in args.seeds.split(",")):
        for name, kw in variants:
            t.manual_seed(0)
            model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
            tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024, seed=seed,
                                 objective="softmax", **kw)
            got = bench.map_at_12(model, tr, inter, held, steps)
            fin = tr.forward()                     # the propagated tables, rows back under their original ids
            if tr.order is not None:
                fin = fin[tr.order.node_new_of_old()]
            full = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], (12, 100),
                                                  embeddings=(fin[:U].contiguous(), fin[U:].contiguous()))
            tr.to_original_order()
            print(json.dumps({"mode": "worth", "variant": name, "trainer_seed": seed, "steps": steps,
                              "propagated_map_at_12": round(got["propagated_embeddings_map_at_12"], 4),
                              "layer0_map_at_12": round(got["value"], 4),
                              "popularity_predictor_map_at_12": round(got["popularity_predictor_map_at_12"], 4),
                              "propagated_full_rank": {k: round(v, 4) for k, v in full.items() if isinstance(v, float)},
                              "final_loss": round(float(tr.loss), 4)}), flush=True)


def every_mode():
    for mode, limit in LIMITS.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), mode]).returncode
        if rc != 0:
            sys.exit(f"{mode} ended with status {rc}: nothing more is started")


{"kernel": kernel, "cost": cost, "worth": worth, "all": every_mode}[args.mode]()
