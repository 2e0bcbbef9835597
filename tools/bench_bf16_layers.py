#!/usr/bin/env python3
"""bf16 layer tables of the LightGCN forward: what the narrower operand buys and what it costs (profiles/bf16_layers.md).

  launch  at C2 (1 M users x 100 K items, 10 M edges, d = 128, K = 3, batch 16 384) under the trainer's locality order:
          ops.rows_to_bf16 of the table; one dense ops.spmm_bf16 launch against one dense ops.spmm launch on the same
          adjacency (ops.spmm with its default plan: the launch as it is without this option, timed in the same run); the
          row-list launch of the last forward layer both ways.  Median of --reps calls after two warm-up rounds, the legs taking
          turns, device events around each call.  --legs picks the legs (for a counter run of one pair on its own).
  step    ms per training step: the sparse-batch step (the default form) and the dense step, each with layer_dtype f32 and
          bf16.  One trainer per leg, the legs' steps INTERLEAVED in one process, events around every step; --runs runs.
  worth   the recipe of profiles/objectives.md section 5: C1-scale planted graph, spec seed 5, D 64, K 2, batch 1024, lr 1e-2,
          lambda 1e-6, 200 steps, trainer seeds 7, 8, 9, propagated predictor: MAP@12, MRR, recall@100 and AUC with f32 and
          bf16 layers under the reference objective and the sampled softmax (M = 4).  Evaluation runs the f32 forward in
          every leg (trainer.forward()).
  pmc     summarises a directory written by `rocprofv3 --pmc FETCH_SIZE -d DIR --output-format csv -- python3
          tools/bench_bf16_layers.py launch --legs dense_f32,dense_bf16`: average FETCH_SIZE per dispatch of every spmm kernel.
--small: C1-sized graph, D 64, K 2: a check that the tool runs, not a measurement.  --graph c4: the C4 graph (100 M edges).
One JSON line per leg.

    python3 tools/bench_bf16_layers.py launch [--reps 11] [--legs convert,dense_f32,dense_bf16,list_f32,list_bf16] [--small]
    python3 tools/bench_bf16_layers.py step [--steps 10] [--warmup 3] [--runs 3] [--legs ...] [--small]
    python3 tools/bench_bf16_layers.py worth [--steps 200] [--seeds 7,8,9]
    python3 tools/bench_bf16_layers.py pmc --dir DIR"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("launch", "step", "worth", "pmc"))
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--legs", default=None)
ap.add_argument("--seeds", default="7,8,9")
ap.add_argument("--graph", choices=("c2", "c4"), default="c2")
ap.add_argument("--dir", default=None)
ap.add_argument("--small", action="store_true", help="a C1-sized graph: a check that the tool runs, not a measurement")
args = ap.parse_args()
DEV = "cuda"


def _setup():
    """(spec, interactions, adjacency, D, K, batch) of the chosen graph."""
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    if args.small:
        spec, D, K, batch = S.C1, 64, 2, min(args.batch, 1024)
        ei = S.generate(spec)
    elif args.graph == "c4":
        spec, D, K, batch = S.C4, 128, 3, args.batch
        ei = S.generate_blocks(spec, S.C4_BLOCKS, 0, S.C4_BLOCKS)
    else:
        spec, D, K, batch = S.C2, 128, 3, args.batch
        ei = S.generate(spec)
    inter = Interactions(ei.to(DEV), spec.num_users, spec.num_items)
    return spec, inter, inter.adjacency("bipartite"), D, K, batch


def _trainer(spec, inter, adj, D, K, batch, **kw):
    import torch as t
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    t.manual_seed(1234)
    model = LightGCN(spec.num_users, spec.num_items, embedding_dim=D, num_iterations=K).to(DEV)
    return LightGCNTrainer(model, adj, inter, lr=1e-3, Lambda=1e-6, batch_size=batch, seed=7, **kw)


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


def launch():
    import torch as t
    from laplace_amd import ops
    spec, inter, adj, D, K, batch = _setup()
    tr = _trainer(spec, inter, adj, D, K, batch)     # the default trainer: its adjacency, order, plan and one batch's node list
    tr.step()
    a, tab, nodes, cnt, c = tr.adj_fwd, tr.table, tr.nodes, tr.n_nodes[:1], 1.0 / (K + 1)
    n, d = tab.shape
    y32 = t.empty_like(tab)
    x0, y16 = t.empty(n, d, dtype=t.bfloat16, device=DEV), t.empty(n, d, dtype=t.bfloat16, device=DEV)
    sum_c, out_c = tr.sum_c, t.empty_like(tr.final_c)
    ops.spmm(a, tab, Y=y32)
    ops.rows_to_bf16(y32, out=y16)                  # the row-list legs read a propagated layer, as the step's last product does
    legs = {"convert": lambda: ops.rows_to_bf16(tab, out=x0),
            "dense_f32": lambda: ops.spmm(a, tab, Y=y32),
            "dense_bf16": lambda: ops.spmm_bf16(a, x0, Y=y16),
            "list_f32": lambda: ops.spmm(a, y32, addend=sum_c, S=out_c, scale=c, row_list=nodes, n_list_dev=cnt),
            "list_bf16": lambda: ops.spmm_bf16(a, y16, addend=sum_c, S=out_c, scale=c, row_list=nodes, n_list_dev=cnt)}
    ops.rows_to_bf16(tab, out=x0)
    if args.legs:
        legs = {k: legs[k] for k in args.legs.split(",")}
    plan = a.plan
    info = {"rows": n, "d": d, "nnz": a.nnz, "reordered": tr.order is not None,
            "f32_plan": None if plan is None else ("sweep" if plan.sweep is not None else f"items band={int(plan.struct.band)}")}
    for name, vals in _timed(legs, args.reps).items():
        print(json.dumps(dict(info, mode="launch", leg=name, ms_median=round(statistics.median(vals), 4),
                              ms_min=round(min(vals), 4), ms_max=round(max(vals), 4), reps=len(vals))), flush=True)
    if a.plan_bf16 is not None:
        st = a.plan_bf16.struct
        print(json.dumps({"mode": "launch", "bf16_plan": f"items band={int(st.band)}", "split_rows": int(st.n_long_rows),
                          "work_items": int(st.n_items)}), flush=True)


def step():
    import torch as t
    steps = args.steps or 10
    spec, inter, adj, D, K, batch = _setup()
    variants = {"sparse_f32": dict(), "sparse_bf16": dict(layer_dtype="bf16"),
                "dense_f32": dict(sparse_batch=False), "dense_bf16": dict(sparse_batch=False, layer_dtype="bf16")}
    keys = args.legs.split(",") if args.legs else list(variants)
    legs = {k: _trainer(spec, inter, adj, D, K, batch, **variants[k]) for k in keys}
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
            print(json.dumps({"mode": "step", "run": run, "leg": name, "batch": batch, "D": D, "K": K, "steps": steps,
                              "ms_per_step_median": round(per[len(per) // 2], 3), "ms_per_step_min": round(per[0], 3),
                              "ms_per_step_max": round(per[-1], 3), "loss": round(float(tr.loss), 5)}), flush=True)


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
        for layer_dtype in ("f32", "bf16"):
            for seed in (int(s) for s in args.seeds.split(",")):
                t.manual_seed(0)
                model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(DEV)
                tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024,
                                     seed=seed, layer_dtype=layer_dtype, **kw)
                got = bench.map_at_12(model, tr, inter, held, steps)
                fin = tr.forward()                     # the f32 propagate, rows back under their original ids
                if tr.order is not None:
                    fin = fin[tr.order.node_new_of_old()]
                full = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], (12, 100),
                                                      embeddings=(fin[:U].contiguous(), fin[U:].contiguous()))
                tr.to_original_order()
                print(json.dumps({"mode": "worth", "objective": objective, "layer_dtype": layer_dtype, "trainer_seed": seed,
                                  "steps": steps, "propagated_map_at_12": round(got["propagated_embeddings_map_at_12"], 4),
                                  "propagated_full_rank": {k: round(v, 4) for k, v in full.items() if isinstance(v, float)},
                                  "final_loss": round(float(tr.loss), 4)}), flush=True)


def pmc():
    files = glob.glob(os.path.join(args.dir, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        sys.exit(f"no counter_collection.csv under {args.dir}")
    agg = collections.defaultdict(list)
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
            if r.get("Counter_Name", "FETCH_SIZE") == "FETCH_SIZE" and "spmm" in name:
                agg[name.split("(")[0][:90]].append(float(r["Counter_Value"]))
    for k, v in sorted(agg.items()):
        print(json.dumps({"mode": "pmc", "kernel": k, "dispatches": len(v), "fetch_size_kib_avg": round(sum(v) / len(v), 1)}),
              flush=True)


{"launch": launch, "step": step, "worth": worth, "pmc": pmc}[args.mode]()
