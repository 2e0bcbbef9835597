#!/usr/bin/env python3
"""PinSAGE evaluation (BASELINE configs[4]) at H&M scale: every item's representation, latest-item
recommendations for every user and hits@K, as pinsage/model.py:120-134 + pinsage/evaluation.py do after each epoch.
Prints one JSON line:
  - the native catalogue pass (mi_pinsage_embed_items_f32), device events, warmed, per walk length;
  - the reference-shaped batched pass (sample_blocks + get_repr per batch of --eval-batch item ids) over the whole catalogue,
    timed once, and its max |difference| to the native pass;
  - LatestNNRecommender.recommend for all users (K10) and users/s;
  - hits@K of the model after --iters native training iterations next to the same model untrained.
The graph and sampler settings are tools/bench_pinsage.py's; each user's last interaction is held out
(data/graph_io.train_test_split_by_time).  --eval-only: the native pass and recommend alone (a profiling run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_371_980)
    ap.add_argument("--items", type=int, default=105_542)
    ap.add_argument("--edges", type=int, default=31_800_000)
    ap.add_argument("--walk-lengths", default="2,3")
    ap.add_argument("--restart", type=float, default=0.5)
    ap.add_argument("--walks", type=int, default=10)
    ap.add_argument("--neighbors", type=int, default=3)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--eval-batch", type=int, default=32)     # pinsage/model.py:148 --batch-size (collate_test's batches)
    ap.add_argument("--train-batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--eval-only", action="store_true")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    import numpy as np
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.graph_io import train_test_split_by_time
    from laplace_amd.pinsage.evaluation import LatestNNRecommender, prec
    from laplace_amd.pinsage.model import PinSAGEModel, train_epoch
    from laplace_amd.pinsage.sampler import PinSAGESampler

    dev = "cuda"
    ei = S.generate(S.SyntheticSpec(args.users, args.items, args.edges, seed=2, zipf_s=1.0))   # tools/bench_pinsage.py's graph
    u, a = ei[0].numpy(), ei[1].numpy()
    _, _, test = train_test_split_by_time(u)          # generation order is the transaction order
    tr = ~test
    users = AdjList.from_edges(u[tr], a[tr], args.users)
    items = AdjList.from_edges(a[tr], u[tr], args.items)
    held = AdjList.from_edges(u[test], a[test], args.users)
    lengths = [int(x) for x in args.walk_lengths.split(",")]
    samplers = {L: PinSAGESampler(users, items, args.users, args.items, batch_size=args.train_batch, random_walk_length=L,
                                  random_walk_restart_prob=args.restart, num_random_walks=args.walks,
                                  num_neighbors=args.neighbors, num_layers=args.layers, seed=1) for L in lengths}
    smp = samplers[lengths[0]]
    t.manual_seed(0)
    model = PinSAGEModel(args.items, args.hidden, args.layers).to(dev)
    out = {"workload": f"PinSAGE evaluation, H&M-shaped synthetic {args.users}x{args.items}, {args.edges} edges (last interaction "
                       f"per user held out: {int(test.sum())}); walks {args.walks}, restart {args.restart}, T={args.neighbors}, "
                       f"{args.layers} layers, hidden {args.hidden}, K={args.k}"}

    def native_ms(s):
        for _ in range(2):
            model.item_representations(s)
        t.cuda.synchronize()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            model.item_representations(s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    rec_engine = LatestNNRecommender()
    for L, s in samplers.items():
        out[f"native_catalogue_pass_ms_walk{L}"] = round(native_ms(s), 3)
    h = model.item_representations(smp)
    rec_engine.recommend(smp, args.k, None, h)        # warm (workspaces, item-side tables)
    t.cuda.synchronize()
    t0 = time.perf_counter()
    recs = rec_engine.recommend(smp, args.k, None, h)
    t.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["recommend_ms_all_users"] = round(1e3 * dt, 2)
    out["recommend_users_per_s"] = round(args.users / dt)
    untrained = prec(recs, held)
    if args.eval_only:
        print(json.dumps(out))
        return

    for L, s in samplers.items():
        step = s.step
        model.eval()
        t.cuda.synchronize()
        t0 = time.perf_counter()
        with t.no_grad():
            ref = model.batched_item_representations(s, step, args.eval_batch)
        t.cuda.synchronize()
        dt = time.perf_counter() - t0
        nat = model.item_representations(s, step=step)
        out[f"batched_pass_s_walk{L}_batch{args.eval_batch}"] = round(dt, 3)
        out[f"native_speedup_walk{L}"] = round(1e3 * dt / out[f"native_catalogue_pass_ms_walk{L}"], 1)
        out[f"max_abs_diff_native_vs_batched_walk{L}"] = float((nat - ref).abs().max())
    model.train()

    opt = t.optim.Adam(model.parameters(), lr=args.lr)
    t.cuda.synchronize()
    t0 = time.perf_counter()
    losses = train_epoch(model, opt, smp, args.iters)
    t.cuda.synchronize()
    out["train"] = {"iters": args.iters, "batch": args.train_batch, "lr": args.lr, "s": round(time.perf_counter() - t0, 2),
                    "loss_first": round(float(np.mean(losses[:20])), 4), "loss_last": round(float(np.mean(losses[-20:])), 4)}
    trained = prec(rec_engine.recommend(smp, args.k, None, model.item_representations(smp)), held)
    out[f"hits@{args.k}_trained"] = round(trained, 5)
    out[f"hits@{args.k}_untrained"] = round(untrained, 5)
    deg = np.diff(users.ptr)
    has = np.diff(held.ptr) > 0
    out[f"hits@{args.k}_uniform_expected"] = round(float(np.mean(np.where(has, args.k / np.maximum(args.items - deg, 1), 0.0))), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
