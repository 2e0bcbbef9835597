#!/usr/bin/env python3
"""The recent-items recommender (DESIGN §7, N5 recent-items recommender): what it costs and what it buys.

Cost.  tools/bench_pinsage.py's H&M-shaped graph, an untrained PinSAGEModel's item representations at --hidden, K = --k:
LatestNNRecommender.recommend (the baseline) against RecentItemsRecommender "mean" and "max" at n_recent 4 and 8, decay 1,
over every user.  The variants live in one process and are timed INTERLEAVED after a warm-up: --reps repetitions of one
recommend() of each in turn, each timed with a device synchronisation around it; the table gives the median with the
min .. max of the repetitions.  Then the three new kernels by themselves, each over every user (the merge: over the real lists
of the first --merge-users users): --reps repetitions of --kernel-calls calls back to back, ms per call.

Effect.  A planted graph in which every user holds TWO communities.  The recipe (fixed before the first run): --fx-items items
in --fx-communities communities of equal size (item i belongs to community i mod communities); user u draws two distinct
communities uniformly and a row length uniformly from --fx-len-min .. --fx-len-max; every entry of the row, in transaction
order, is with probability --fx-mix a uniform item of one of the user's two communities (either with probability 1/2,
independently per entry) and a uniform item of the catalogue otherwise.  The last entry of every row is held out, the rest
is the training graph.  PinSAGEModel trained for --epochs x --epoch-iters native iterations; hits@10 of the latest-item
recommender and of "mean" / "max" at n_recent 4 and 8 (decay 1) and at n_recent 8 with decay 0.8, per seed (graph,
initialisation and batches all follow it).

Prints one JSON line; --markdown PATH writes the tables."""
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
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--merge-users", type=int, default=262_144)
    ap.add_argument("--kernel-calls", type=int, default=20)
    ap.add_argument("--fx-users", type=int, default=6000)
    ap.add_argument("--fx-items", type=int, default=2000)
    ap.add_argument("--fx-communities", type=int, default=20)
    ap.add_argument("--fx-len-min", type=int, default=8)
    ap.add_argument("--fx-len-max", type=int, default=24)
    ap.add_argument("--fx-mix", type=float, default=0.9)
    ap.add_argument("--fx-batch", type=int, default=64)
    ap.add_argument("--fx-hidden", type=int, default=32)
    ap.add_argument("--fx-lr", type=float, default=3e-3)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--epoch-iters", type=int, default=2000)
    ap.add_argument("--seeds", default="1,2,3")
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--time-limit", type=int, default=1100)
    return ap.parse_args(argv)


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _timed(fn, t, calls=1):
    """ms per call of `calls` calls back to back, a device synchronisation before and after."""
    t.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def cost(args) -> dict:
    import torch as t
    from laplace_amd import ops, synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.evaluation import LatestNNRecommender, RecentItemsRecommender
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.sampler import PinSAGESampler
    dev = "cuda"
    ei = S.generate(S.SyntheticSpec(args.users, args.items, args.edges, seed=2, zipf_s=1.0))   # tools/bench_pinsage.py's graph
    u, a = ei[0].numpy(), ei[1].numpy()
    users, items = AdjList.from_edges(u, a, args.users), AdjList.from_edges(a, u, args.items)
    smp = PinSAGESampler(users, items, args.users, args.items, batch_size=32, seed=1)
    t.manual_seed(0)
    model = PinSAGEModel(args.items, args.hidden, 2).to(dev)
    h = model.item_representations(smp, step=0)
    K = args.k
    variants = {"latest item": LatestNNRecommender()}
    for pool in ("mean", "max"):
        for n in (4, 8):
            variants[f"{pool}, n_recent {n}"] = RecentItemsRecommender(n, pool, 1.0)
    times = {name: [] for name in variants}
    for rep in range(args.warmup + args.reps):
        for name, rec in variants.items():
            ms = _timed(lambda: rec.recommend(smp, K, None, h), t)
            if rep >= args.warmup:
                times[name].append(ms)
    # the kernels by themselves
    kernels = {}
    ptr, idx = smp.ui_ptr, smp.ui_idx
    for n in (4, 8):
        rec = RecentItemsRecommender(n, "max", 1.0)
        w = t.from_numpy(rec.weights()).to(dev)
        its, n_slots = ops.recent_items(ptr, idx, n)
        m = min(args.merge_users, args.users)
        excl = ops.row_slice(ops.DeviceCSR(args.users, args.items, ptr, idx), 0, m)
        lists = [ops.topk_excl(its[r, :m], h, h, K, excl, want_scores=True) for r in range(n)]
        ids, sc = t.stack([l[0] for l in lists]), t.stack([l[1] for l in lists])
        calls = {f"mi_recent_items, n_recent {n}, {args.users} users": lambda: ops.recent_items(ptr, idx, n),
                 f"mi_pool_recent_f32, n_recent {n}, d {args.hidden}, {args.users} users": lambda: ops.pool_recent(its, n_slots, w, h),
                 f"mi_topk_merge_max_f32, {n} lists x {K}, {m} users": lambda: ops.topk_merge_max(ids, sc, n_slots[:m], w, K)}
        for name, fn in calls.items():
            fn()
            kernels[name] = _stat([_timed(fn, t, args.kernel_calls) for _ in range(args.reps)])
        kernels[f"mean slots per user, n_recent {n}"] = round(float(n_slots.float().mean()), 3)
        del lists, ids, sc, its
    return {"workload": f"H&M-shaped synthetic {args.users}x{args.items}, {args.edges} edges; untrained PinSAGEModel representations, "
                        f"hidden {args.hidden}; K = {K}; every user; {args.reps} interleaved repetitions after {args.warmup} warm-up",
            "rows": {name: _stat(ms) for name, ms in times.items()}, "kernels": kernels, "users": args.users}


def two_community_graph(args, seed):
    """The recipe of the module docstring: (user ids, item ids) of every entry in transaction order, and every user's two
    communities."""
    import numpy as np
    rng = np.random.default_rng(seed)
    U, I, C = args.fx_users, args.fx_items, args.fx_communities
    per = I // C
    first = rng.integers(0, C, U)
    second = (first + rng.integers(1, C, U)) % C                      # distinct from the first
    lens = rng.integers(args.fx_len_min, args.fx_len_max + 1, U)
    u = np.repeat(np.arange(U), lens)
    own = rng.random(u.size) < args.fx_mix
    which = np.where(rng.random(u.size) < 0.5, first[u], second[u])
    in_community = which + C * rng.integers(0, per, u.size)           # item i belongs to community i mod C
    anywhere = rng.integers(0, I, u.size)
    return u, np.where(own, in_community, anywhere), np.stack([first, second], 1)


def effect(args) -> dict:
    import numpy as np
    import torch as t
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.evaluation import LatestNNRecommender, RecentItemsRecommender, evaluate_nn
    from laplace_amd.pinsage.model import PinSAGEModel, train_epoch
    from laplace_amd.pinsage.sampler import PinSAGESampler
    dev = "cuda"
    U, I = args.fx_users, args.fx_items
    recs = {"latest item": LatestNNRecommender()}
    for pool in ("mean", "max"):
        for n, decay in ((4, 1.0), (8, 1.0), (8, 0.8)):
            recs[f"{pool}, n_recent {n}, decay {decay}"] = RecentItemsRecommender(n, pool, decay)
    seeds = [int(s) for s in args.seeds.split(",")]
    rows = {name: [] for name in recs}
    untrained, same_community, loss_first, loss_last = [], [], [], []
    for seed in seeds:
        u, a, comm = two_community_graph(args, seed)
        last = np.r_[u[1:] != u[:-1], True]                            # the last entry of every row is held out
        tr = ~last
        users, items = AdjList.from_edges(u[tr], a[tr], U), AdjList.from_edges(a[tr], u[tr], I)
        held = AdjList.from_edges(u[last], a[last], U)
        C = args.fx_communities
        latest_train = a[tr][np.r_[u[tr][1:] != u[tr][:-1], True]]
        same_community.append(float(np.mean(latest_train % C == a[last] % C)))
        smp = PinSAGESampler(users, items, U, I, batch_size=args.fx_batch, seed=seed)
        t.manual_seed(seed)
        model = PinSAGEModel(I, args.fx_hidden, 2).to(dev)
        untrained.append(evaluate_nn(model, smp, held, 10))
        opt = t.optim.Adam(model.parameters(), lr=args.fx_lr)
        for e in range(args.epochs):
            losses = train_epoch(model, opt, smp, args.epoch_iters)
            if e == 0:
                loss_first.append(float(np.mean(losses)))
        loss_last.append(float(np.mean(losses)))
        step = smp.step
        for name, rec in recs.items():
            rows[name].append(evaluate_nn(model, smp, held, 10, step=step, recommender=rec))
    return {"workload": f"two communities per user: {U} users x {I} items, {args.fx_communities} communities of "
                        f"{I // args.fx_communities} items, rows of {args.fx_len_min} .. {args.fx_len_max} entries, mix {args.fx_mix}; "
                        f"every user's last entry held out; hidden {args.fx_hidden}, 2 layers, batch {args.fx_batch}, Adam lr "
                        f"{args.fx_lr}, {args.epochs} epochs x {args.epoch_iters} native iterations; seeds {seeds}",
            "hits_untrained": untrained, "hits_uniform_recommender": 10.0 / I, "latest_in_held_out_community": same_community,
            "loss_first": loss_first, "loss_last": loss_last, "rows": rows}


def markdown(out) -> str:
    lines = ["# PinSAGE recent-items recommender (tools/bench_pinsage_recent.py)", ""]
    if "cost" in out:
        cst = out["cost"]
        cell = lambda s: f"{s['ms']:.2f} ({s['min']:.2f} .. {s['max']:.2f})"
        cell3 = lambda s: f"{s['ms']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"
        base = cst["rows"]["latest item"]["ms"]
        lines += ["## Cost", "", cst["workload"] + ".", "",
                  "`recommend()` over every user: ms, median of the repetitions (min .. max), users per second at the median, and the "
                  "median as a multiple of the latest-item recommender's.", "",
                  "| recommender | ms | users/s | x latest |", "|---|---|---:|---:|"]
        for name, r in cst["rows"].items():
            lines.append(f"| {name} | {cell(r)} | {cst['users'] / r['ms'] * 1e3 / 1e6:.2f} M | {r['ms'] / base:.2f} |")
        lines += ["", "The new kernels by themselves (ms per call, calls back to back between two synchronisations; median (min .. max) of the repetitions):", "",
                  "| call | ms |", "|---|---|"]
        for name, r in cst["kernels"].items():
            lines.append(f"| {name} | {cell3(r) if isinstance(r, dict) else r} |")
        lines.append("")
    if "effect" in out:
        fx = out["effect"]
        mean = lambda xs: sum(xs) / len(xs)
        per = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
        lines += ["## Effect", "", fx["workload"] + ".", "",
                  f"hits@10 untrained (latest item): {per(fx['hits_untrained'])}; a uniform recommender: about "
                  f"{fx['hits_uniform_recommender']:.4f}.  Share of users whose latest training item lies in the held-out item's "
                  f"community: {per(fx['latest_in_held_out_community'])}.  Mean loss of the first epoch: {per(fx['loss_first'])}; of the "
                  f"last: {per(fx['loss_last'])}.", "",
                  "| recommender | hits@10 per seed | mean |", "|---|---|---:|"]
        for name, r in fx["rows"].items():
            lines.append(f"| {name} | {per(r)} | {mean(r):.3f} |")
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
    path = args.markdown or os.path.join(ROOT, "profiles", "pinsage_recent_items.md")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
