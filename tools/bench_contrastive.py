#!/usr/bin/env python3
"""The noise-view contrastive term of the LightGCN trainer: what it costs and what it is worth (profiles/contrastive.md).

  kernel  ops.perturb_rows (with addend / S, the trainer's form) and ops.adam_step on [N, d] tables at C2's size (1.1 M rows,
          d = 128): median of --reps calls after a warm-up, the two taking turns, device events around each call; ms and the
          achieved bytes per second of the bytes each must move (perturb: read X and addend, write X and S, 4 N d 4; Adam:
          read p, g, m, v, write p, m, v, 7 N d 4).  ops.contrastive_fwd_bwd and ops.inbatch_softmax_fwd_bwd at B = 16 384,
          the same group, on the same tables, in turn as well.
  cost    ms per training step at C2 (1 M users x 100 K items, 10 M edges, D = 128, K = 3, batch 16 384), sparse_batch=False,
          reference objective, one negative: cl_weight = 0 (the step as it is launched without the keywords) against
          cl_weight = 0.2.  One trainer per leg, the legs' steps INTERLEAVED in one process, events around every step; --runs
          runs per leg.  --legs picks the legs (for a kernel trace of one leg in a run of its own).
  worth   the recipe of profiles/objectives.md section 5: C1-scale planted graph, spec seed 5, D 64, K 2, batch 1024, lr 1e-2,
          lambda 1e-6, 200 steps, bench.map_at_12, trainer seeds 7, 8, 9.  cl_weight in {0, 0.05, 0.2} at the default eps, tau,
          layer and group, under objective="softmax", n_neg=4 and under the reference objective; the dense step in every leg.
          Propagated MAP@12 and full_rank_metrics of the propagated tables on the held-out edges (recall@100, MRR, AUC).
  all     the three modes as child processes, each under its own time limit, stopping at the first that does not end well.
One JSON line per leg.

    python3 tools/bench_contrastive.py kernel [--rows 1100000] [--d 128] [--reps 11]
    python3 tools/bench_contrastive.py cost [--steps 10] [--warmup 3] [--runs 3] [--legs off,on] [--small]
    python3 tools/bench_contrastive.py worth [--steps 200] [--seeds 7,8,9]
    python3 tools/bench_contrastive.py all"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"kernel": 300, "cost": 600, "worth": 600}   # seconds a mode may take as a child of `all`

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("kernel", "cost", "worth", "all"))
ap.add_argument("--rows", type=int, default=1_100_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--group", type=int, default=1024)
ap.add_argument("--legs", default="off,on")
ap.add_argument("--seeds", default="7,8,9")
ap.add_argument("--small", action="store_true", help="cost on a C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
DEV = "cuda"


def _timed(legs, reps):
    """{name: [ms]}: the legs take turns inside every repetition, after two warm-up rounds."""
    import torch as t
    ms = {name: [] for name in legs}
    for rep in range(reps + 2):
        for name, fn in legs.items():
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[name].append(a.elapsed_time(b))
    return ms


def kernel():
    import torch as t
    from laplace_amd import ops
    N, d, B, G = args.rows, args.d, args.batch, args.group
    g = t.Generator(device=DEV).manual_seed(0)
    x, addend, s = (t.randn(N, d, device=DEV, generator=g) * 0.1 for _ in range(3))
    p, grad, m, v = (t.randn(N, d, device=DEV, generator=g) * 0.1 for _ in range(4))
    v.abs_()
    ids = t.randint(0, N, (B,), device=DEV, generator=g)
    users, pos = t.randint(0, N // 2, (B,), device=DEV, generator=g), t.randint(0, N // 2, (B,), device=DEV, generator=g)
    g_a, g_b, rw, out = t.zeros(N, d, device=DEV), t.zeros(N, d, device=DEV), t.zeros(N, device=DEV), t.zeros(1, device=DEV)
    legs = {"perturb_rows (addend, S)": lambda: ops.perturb_rows(x, eps=0.2, layer=1, seed=1, step=0, addend=addend, S=s),
            "adam_step": lambda: ops.adam_step(p, grad, m, v, step=1, lr=1e-3),
            "contrastive_fwd_bwd": lambda: ops.contrastive_fwd_bwd(ids, x, addend, tau=0.15, group=G, g_a=g_a, g_b=g_b,
                                                                   loss_out=out),
            "inbatch_softmax_fwd_bwd": lambda: ops.inbatch_softmax_fwd_bwd(users, pos, x, x, N // 2, 1e-6, group=G, g_final=g_a,
                                                                           reg_w=rw, loss_out=out)}
    nbytes = {"perturb_rows (addend, S)": 4 * N * d * 4, "adam_step": 7 * N * d * 4}
    for name, vals in _timed(legs, args.reps).items():
        med = statistics.median(vals)
        line = {"mode": "kernel", "leg": name, "rows": N, "d": d, "batch": B, "group": G, "ms_median": round(med, 4),
                "ms_min": round(min(vals), 4), "ms_max": round(max(vals), 4), "reps": len(vals)}
        if name in nbytes:
            line.update(bytes=nbytes[name], tb_per_s=round(nbytes[name] / (med * 1e-3) / 1e12, 3))
        print(json.dumps(line), flush=True)


def cost():
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    steps = args.steps or 10
    spec = S.C1 if args.small else S.C2
    D, K = (64, 2) if args.small else (128, 3)
    batch = min(args.batch, 1024) if args.small else args.batch
    inter = Interactions(S.generate(spec).to(DEV), spec.num_users, spec.num_items)
    adj = inter.adjacency("bipartite")
    variants = {"off": ("dense step, cl_weight=0", dict()),
                "on": ("dense step, cl_weight=0.2", dict(cl_weight=0.2, cl_group=min(args.group, 1024)))}
    legs = {}
    for key in args.legs.split(","):
        name, kw = variants[key]
        t.manual_seed(1234)
        model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to(DEV)
        legs[name] = LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=batch, seed=7, sparse_batch=False, **kw)
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
            print(json.dumps({"mode": "cost", "run": run, "leg": name, "objective": "reference", "sparse_batch": False,
                              "batch": batch, "steps": steps, "ms_per_step_median": round(per[len(per) // 2], 3),
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
    U = spec.num_users
    for objective, kw in (("softmax, M=4", dict(objective="softmax", n_neg=4)), ("reference", dict(objective="reference"))):
        for weight in (0.0, 0.05, 0.2):
            for seed in (int(s) for s in args.seeds.split(",")):
                t.manual_seed(0)
                model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
                tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024,
                                     seed=seed, sparse_batch=False, cl_weight=weight, **kw)
                got = bench.map_at_12(model, tr, inter, held, steps)
                fin = tr.forward()                     # the unperturbed propagate, rows back under their original ids
                if tr.order is not None:
                    fin = fin[tr.order.node_new_of_old()]
                full = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], (12, 100),
                                                      embeddings=(fin[:U].contiguous(), fin[U:].contiguous()))
                tr.to_original_order()
                print(json.dumps({"mode": "worth", "objective": objective, "cl_weight": weight, "trainer_seed": seed,
                                  "steps": steps, "propagated_map_at_12": round(got["propagated_embeddings_map_at_12"], 4),
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
