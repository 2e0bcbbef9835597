#!/usr/bin/env python3
"""Hard negatives from random-walk ranks (DESIGN §7, N5 hard negatives): what they cost and what they buy.

Cost.  tools/bench_pinsage.py's H&M-shaped graph and the reference's settings (batch 32, hidden 16, 10 walks of length 2,
T = 3, 2 layers): one native iteration through PinSAGESampler.batches(), the uniform sampler against
HardNegatives(--hard-walks, --hard-length, --hard-restart, --cost-window) at share = 1.  The variants — uniform, hard, and a
second uniform instance that shows what two instances of one configuration differ by — live in one process and are timed
INTERLEAVED after a warm-up: --reps repetitions of --iters iterations of each in turn, each timed with a device synchronisation
around it; the table gives the median with the min .. max of the repetitions.  The same for the sampler
chain alone — sample_batch() by itself (one chain's latency) and batches() with nothing to train (the period of two chains side
by side) — since the extra launch lengthens a latency chain that runs beside the training step.

Effect.  A planted-community graph (synthetic.SyntheticSpec.communities), every user's latest interaction held out
(data/graph_io.train_test_split_by_time), PinSAGEModel trained for --epochs x --epoch-iters native iterations per variant:
uniform negatives, share = 0.5, and a curriculum whose share rises linearly from 0 to 0.75 over the epochs.  The rank window is
set from the community size c = items / communities: [c / 4, c).  Per seed (graph, initialisation and batches all follow it):
hits@10 of evaluate_nn, and the share of pairs whose hinge is non-zero at the end of training, in eval mode over --probe
fresh batches, against uniform negatives and against the variant's own negatives.

Prints one JSON line; --markdown PATH writes the two tables."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="cost,effect")
    ap.add_argument("--users", type=int, default=1_371_980)
    ap.add_argument("--items", type=int, default=105_542)
    ap.add_argument("--edges", type=int, default=31_800_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--hard-walks", type=int, default=256)
    ap.add_argument("--hard-length", type=int, default=2)
    ap.add_argument("--hard-restart", type=float, default=0.5)
    ap.add_argument("--cost-window", default="10,50")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fx-users", type=int, default=6000)
    ap.add_argument("--fx-items", type=int, default=2000)
    ap.add_argument("--fx-edges", type=int, default=120_000)
    ap.add_argument("--fx-communities", type=int, default=20)
    ap.add_argument("--fx-mix", type=float, default=0.85)
    ap.add_argument("--fx-batch", type=int, default=64)
    ap.add_argument("--fx-hidden", type=int, default=32)
    ap.add_argument("--fx-lr", type=float, default=3e-3)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--epoch-iters", type=int, default=150)
    ap.add_argument("--seeds", default="1,2,3")
    ap.add_argument("--probe", type=int, default=50)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--time-limit", type=int, default=1100)
    return ap.parse_args(argv)


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def cost(args) -> dict:
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import HardNegatives, PinSAGESampler
    dev = "cuda"
    ei = S.generate(S.SyntheticSpec(args.users, args.items, args.edges, seed=2, zipf_s=1.0))   # tools/bench_pinsage.py's graph
    u, a = ei[0].numpy(), ei[1].numpy()
    users, items = AdjList.from_edges(u, a, args.users), AdjList.from_edges(a, u, args.items)
    lo, hi = (int(x) for x in args.cost_window.split(","))
    variants = {}
    for which in ("uniform", "hard", "uniform again"):      # the third: a second uniform instance, the instance-to-instance floor
        hn = HardNegatives(args.hard_walks, args.hard_length, args.hard_restart, lo, hi, 1.0) if which == "hard" else None
        smp = PinSAGESampler(users, items, args.users, args.items, batch_size=args.batch, seed=1, hard_negatives=hn)
        t.manual_seed(0)
        model = PinSAGEModel(args.items, args.hidden, 2).to(dev)
        opt = t.optim.Adam(model.parameters(), lr=3e-5, fused=True)       # tools/bench_pinsage.py's optimizer
        model.train()
        native = NativePinSAGEStep(model, opt)
        for _ in range(args.warmup):
            assert native.step(smp.sample_batch()) is not None, native.declined
        for _ in smp.batches(args.warmup):
            pass
        t.cuda.synchronize()
        variants[which] = dict(smp=smp, native=native, iteration=[], chain=[], period=[])
    taken = int((variants["hard"]["smp"].hard_negative_ranks(0) >= 0).sum())
    for _ in range(args.reps):
        for which, v in variants.items():
            smp, native = v["smp"], v["native"]
            t.cuda.synchronize()
            t0 = time.perf_counter()
            for b in smp.batches(args.iters):
                assert native.step(b) is not None, native.declined
            t.cuda.synchronize()
            v["iteration"].append(1e3 * (time.perf_counter() - t0) / args.iters)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                smp.sample_batch()                      # synchronises on its counts: one chain's latency
            t.cuda.synchronize()
            v["chain"].append(1e3 * (time.perf_counter() - t0) / args.iters)
            t0 = time.perf_counter()
            for _ in smp.batches(args.iters):
                pass
            t.cuda.synchronize()
            v["period"].append(1e3 * (time.perf_counter() - t0) / args.iters)
    return {"workload": f"H&M-shaped synthetic {args.users}x{args.items}, {args.edges} edges; batch {args.batch} pairs, 10 walks x length "
                        f"2, restart 0.5, T=3, 2 layers, hidden {args.hidden}; hard negatives: {args.hard_walks} walks x length "
                        f"{args.hard_length}, restart {args.hard_restart}, ranks [{lo}, {hi}), share 1 ({taken} of {args.batch} pairs of "
                        f"batch 0 took a hard negative); {args.reps} interleaved repetitions of {args.iters} iterations after "
                        f"{args.warmup} warm-up iterations",
            "rows": {which: {k: _stat(v[k]) for k in ("iteration", "chain", "period")} for which, v in variants.items()}}


def effect(args) -> dict:
    import numpy as np
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.graph_io import train_test_split_by_time
    from laplace_amd.pinsage.evaluation import evaluate_nn
    from laplace_amd.pinsage.model import PinSAGEModel, train_epoch
    from laplace_amd.pinsage.sampler import HardNegatives, PinSAGESampler
    dev = "cuda"
    U, I, K = args.fx_users, args.fx_items, args.fx_communities
    c = I // K
    lo, hi = max(c // 4, 1), c
    schedules = {"uniform": lambda e: None, "share 0.5": lambda e: 0.5,
                 "curriculum 0 -> 0.75": lambda e: 0.75 * e / max(args.epochs - 1, 1)}
    seeds = [int(s) for s in args.seeds.split(",")]
    rows = {name: {"hits": [], "hinge_uniform": [], "hinge_own": [], "loss_last": []} for name in schedules}
    untrained = []
    for seed in seeds:
        ei = S.generate(S.SyntheticSpec(U, I, args.fx_edges, seed=seed, communities=K, community_mix=args.fx_mix))
        u, a = ei[0].numpy(), ei[1].numpy()
        _, _, test = train_test_split_by_time(u)            # generation order is the transaction order
        tr = ~test
        users, items = AdjList.from_edges(u[tr], a[tr], U), AdjList.from_edges(a[tr], u[tr], I)
        held = AdjList.from_edges(u[test], a[test], U)
        mk = lambda sd, hn=None: PinSAGESampler(users, items, U, I, batch_size=args.fx_batch, seed=sd, hard_negatives=hn)
        for name, share_of in schedules.items():
            hn = None if share_of(0) is None else HardNegatives(args.hard_walks, args.hard_length, args.hard_restart, lo, hi, 0.0)
            smp = mk(seed, hn)
            t.manual_seed(seed)
            model = PinSAGEModel(I, args.fx_hidden, 2).to(dev)
            if name == "uniform":
                untrained.append(evaluate_nn(model, smp, held, 10))
            opt = t.optim.Adam(model.parameters(), lr=args.fx_lr)
            for e in range(args.epochs):
                if hn is not None:
                    hn.share = share_of(e)
                losses = train_epoch(model, opt, smp, args.epoch_iters)
            r = rows[name]
            r["loss_last"].append(float(np.mean(losses)))
            r["hits"].append(evaluate_nn(model, smp, held, 10))
            model.eval()
            probes = {"hinge_uniform": mk(seed + 1000)}
            probes["hinge_own"] = mk(seed + 1000, hn) if hn is not None else probes["hinge_uniform"]
            with t.no_grad():
                for key, ps in probes.items():
                    live = total = 0
                    for step in range(args.probe):
                        b = ps.sample_batch(step)
                        hinge = model(b["seeds"], b["pos"], b["neg"], b["blocks"])
                        live += int((hinge > 0).sum())
                        total += hinge.numel()
                    r[key].append(live / max(total, 1))
            model.train()
    deg_free = 10.0 / I
    return {"workload": f"planted communities: {U} users x {I} items, {args.fx_edges} edges, {K} communities of {c} items, mix "
                        f"{args.fx_mix}; every user's latest interaction held out; hidden {args.fx_hidden}, 2 layers, batch "
                        f"{args.fx_batch}, Adam lr {args.fx_lr}, {args.epochs} epochs x {args.epoch_iters} native iterations; hard "
                        f"negatives: {args.hard_walks} walks x length {args.hard_length}, restart {args.hard_restart}, ranks [{lo}, {hi}); "
                        f"seeds {seeds}; hinge shares in eval mode over {args.probe} fresh batches",
            "hits_untrained": untrained, "hits_uniform_recommender": deg_free, "rows": rows}


def markdown(out) -> str:
    lines = ["# PinSAGE hard negatives from random-walk ranks (tools/bench_pinsage_hard.py)", ""]
    if "cost" in out:
        cst = out["cost"]
        cell = lambda s: f"{s['ms']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"
        lines += ["## Cost", "", cst["workload"] + ".", "",
                  "ms, median of the repetitions (min .. max).  iteration: one native training iteration through `batches()`; chain: "
                  "`sample_batch()` alone (one chain's latency, the count read-back included); period: `batches()` with nothing to "
                  "train (two chains side by side).", "",
                  "| negatives | iteration | chain | period |", "|---|---|---|---|"]
        for which, r in cst["rows"].items():
            lines.append(f"| {which} | {cell(r['iteration'])} | {cell(r['chain'])} | {cell(r['period'])} |")
        a = cst["rows"]["uniform"]
        lines += ["", "`uniform again` is a second sampler / model / executor of the uniform kind built after the other two: what two "
                  "instances of one configuration differ by in this process.", ""]
        for other in ("hard", "uniform again"):
            b = cst["rows"][other]
            for k in ("iteration", "chain", "period"):
                spread = max(a[k]["max"] - a[k]["min"], b[k]["max"] - b[k]["min"])
                lines.append(f"- {k}: {other} - uniform = {b[k]['ms'] - a[k]['ms']:+.3f} ms ({100 * (b[k]['ms'] - a[k]['ms']) / a[k]['ms']:+.1f} %), "
                             f"run-to-run spread {spread:.3f} ms.")
        lines.append("")
    if "effect" in out:
        fx = out["effect"]
        mean = lambda xs: sum(xs) / len(xs)
        per = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
        lines += ["## Effect", "", fx["workload"] + ".", "",
                  f"hits@10 untrained: {per(fx['hits_untrained'])}; a uniform recommender: about {fx['hits_uniform_recommender']:.4f}.", "",
                  "Per seed, then the mean.  live hinge: share of pairs with hinge > 0 at the end of training.", "",
                  "| negatives | hits@10 per seed | mean | live hinge, uniform negatives | mean | live hinge, own negatives | mean | last-epoch loss |",
                  "|---|---|---:|---|---:|---|---:|---:|"]
        for name, r in fx["rows"].items():
            lines.append(f"| {name} | {per(r['hits'])} | {mean(r['hits']):.3f} | {per(r['hinge_uniform'])} | {mean(r['hinge_uniform']):.3f} | "
                         f"{per(r['hinge_own'])} | {mean(r['hinge_own']):.3f} | {mean(r['loss_last']):.3f} |")
        lines.append("")
    return "\n".join(lines)


def main():
    args = parse_args()
    signal.alarm(args.time_limit)          # SIGALRM's default action ends the process: the tool's own time limit
    import torch as t
    t.autograd.set_multithreading_enabled(False)
    out = {}
    parts = args.part.split(",")
    if "effect" in parts:
        out["effect"] = effect(args)
        print(json.dumps(out["effect"]), file=sys.stderr, flush=True)
    if "cost" in parts:
        out["cost"] = cost(args)
    path = args.markdown or os.path.join(ROOT, "profiles", "pinsage_hard_negatives.md")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
