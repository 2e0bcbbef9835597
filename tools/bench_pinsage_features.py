#!/usr/bin/env python3
"""PinSAGE with item features (BASELINE configs[4]) at the H&M shape: one training iteration and one catalogue
pass for the three model kinds — id only, features only, id + features — at hidden 16 and 128.  The graph and the sampler
settings are tools/bench_pinsage.py's (synthetic.C3's 1.37 M users x 105 542 items, 31.8 M edges; batch 32, 10 walks of length
2, restart 0.5, T = 3, 2 layers); the item features are synthetic.generate_hetero's article columns (HM_ARTICLE_CARDS =
47 224 / 132 / 30 / 50 values, drawn the same way).  Prints one JSON line.  --kinds / --hiddens narrow the run (a profiling
run of one kind); --time-limit ends the process by itself after that many seconds.  --text N adds N bag-of-words text columns
(TextColumn: vocabulary --text-vocab, lengths uniform over 0 .. 2 x --text-len, so --text-len is the mean) to the feature sets."""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("id", "features", "id+features")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_371_980)
    ap.add_argument("--items", type=int, default=105_542)
    ap.add_argument("--edges", type=int, default=31_800_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--walk-length", type=int, default=2)
    ap.add_argument("--restart", type=float, default=0.5)
    ap.add_argument("--walks", type=int, default=10)
    ap.add_argument("--neighbors", type=int, default=3)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--hiddens", default="16,128")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--dense", type=int, default=0, help="float feature columns beside the four categorical ones")
    ap.add_argument("--text", type=int, default=0, help="bag-of-words text columns beside the other features (at most 4)")
    ap.add_argument("--text-len", type=int, default=8, help="mean bag length (lengths are uniform over 0 .. 2 x this)")
    ap.add_argument("--text-vocab", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--time-limit", type=int, default=540)
    return ap.parse_args(argv)


def main():
    args = parse_args()
    signal.alarm(args.time_limit)          # SIGALRM's default action ends the process: the tool's own time limit
    import numpy as np
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel, TextColumn
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler

    dev = "cuda"
    ei = S.generate(S.SyntheticSpec(args.users, args.items, args.edges, seed=2, zipf_s=1.0))   # tools/bench_pinsage.py's graph
    u, a = ei[0].numpy(), ei[1].numpy()
    users, items = AdjList.from_edges(u, a, args.users), AdjList.from_edges(a, u, args.items)
    rng = np.random.default_rng(2 + 7919)                                                      # generate_hetero's article columns
    cards = S.HM_ARTICLE_CARDS
    ax = np.stack([rng.integers(0, min(c, args.items) if c > 1000 else c, size=args.items) for c in cards], 1)
    dense = t.from_numpy(rng.standard_normal((args.items, args.dense)).astype(np.float32)).to(dev) if args.dense else None
    text = []
    for _ in range(args.text):
        lens = rng.integers(0, 2 * args.text_len + 1, size=args.items)
        toks = rng.integers(0, args.text_vocab, size=(args.items, max(1, 2 * args.text_len)))
        text.append(TextColumn(t.from_numpy(toks), t.from_numpy(lens), args.text_vocab).to(dev))
    feats = ItemFeatures(t.from_numpy(ax.astype(np.int64)).to(dev), dense, cardinalities=cards, text=text)
    out = {"workload": f"PinSAGE with item features, H&M-shaped synthetic {args.users}x{args.items}, {args.edges} edges; batch "
                       f"{args.batch} pairs, walks {args.walks} x length {args.walk_length}, restart {args.restart}, "
                       f"T={args.neighbors}, {args.layers} layers; categorical columns {cards}, {args.dense} float columns, "
                       f"{args.text} text columns (mean length {args.text_len}, vocabulary {args.text_vocab})",
           "results": []}
    t.autograd.set_multithreading_enabled(False)
    for hidden in (int(h) for h in args.hiddens.split(",")):
        for kind in args.kinds.split(","):
            kw = {"id": {}, "features": dict(features=feats, use_id=False), "id+features": dict(features=feats)}[kind]
            smp = PinSAGESampler(users, items, args.users, args.items, batch_size=args.batch, random_walk_length=args.walk_length,
                                 random_walk_restart_prob=args.restart, num_random_walks=args.walks,
                                 num_neighbors=args.neighbors, num_layers=args.layers, seed=1)
            t.manual_seed(0)
            model = PinSAGEModel(args.items, hidden, args.layers, **kw).to(dev)
            opt = t.optim.Adam(model.parameters(), lr=3e-5, fused=True)          # tools/bench_pinsage.py's optimizer
            model.train()
            native = NativePinSAGEStep(model, opt)
            for _ in range(10):
                assert native.step(smp.sample_batch()) is not None, native.declined
            t.cuda.synchronize()
            t0 = time.perf_counter()
            for b in smp.batches(args.iters):
                loss = native.step(b)
                assert loss is not None, native.declined
            t.cuda.synchronize()
            ms_iter = 1e3 * (time.perf_counter() - t0) / args.iters
            row = {"kind": kind, "hidden": hidden, "ms_per_iteration": round(ms_iter, 3), "loss": round(float(loss), 4)}
            if args.reps > 0:                  # --reps 0: the iteration alone (a kernel trace of it)
                for _ in range(2):
                    model.item_representations(smp)
                t.cuda.synchronize()
                e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    h = model.item_representations(smp)
                e1.record()
                e1.synchronize()
                row.update(catalogue_pass_ms=round(e0.elapsed_time(e1) / args.reps, 3), finite=bool(t.isfinite(h).all()))
            out["results"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
