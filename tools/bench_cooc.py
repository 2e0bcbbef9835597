"""Measures the scored item co-occurrence matcher (csrc/cooccurrence.hip) at the H&M shape and writes profiles/cooc_matcher.md:

  * stage 1 (mi_cooc_items_topt, T = 32, cosine) and stage 2 (mi_match_cooc_i32, every user, k = 20 and 100) in
    milliseconds from HIP events after a warm-up, on synthetic.C3 (1 371 980 x 105 542, 31.8 M edges); beside them, for
    scale only, UsersWithCommonItemsMatcher's device form (mi_match_common_items_i32) at the same k;
  * per-kernel times from ONE `rocprofv3 --kernel-trace --stats` run of a child process of this file (a run of its own:
    tracing slows the host, the event times above are taken with the profiler off);
  * candidate recall of [LightGCN, popular] against [LightGCN, popular, co-occurrence] on synthetic.heldout_edges, on C3
    (no planted structure: nothing to learn beyond popularity) and on the planted graph of tools/e2e_hm_scale.py (same
    shape, 32 user / item groups).

    python tools/bench_cooc.py [--out profiles/cooc_matcher.md] [--no-trace] [--recall c3,planted] [--small]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T_NEIGHBORS = 32
KS = (20, 100)


def device_csr(ei_np, U, I, dev="cuda"):
    """(users AdjList, articles AdjList, (uptr, uidx, aptr, aidx) int32 on the device), list order = edge order."""
    import numpy as np
    import torch as t
    from laplace_amd.data.dataset import AdjList
    users, articles = AdjList.from_edges(ei_np[0], ei_np[1], U), AdjList.from_edges(ei_np[1], ei_np[0], I)
    to32 = lambda a: t.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
    return users, articles, (to32(users.ptr), to32(users.idx), to32(articles.ptr), to32(articles.idx))


def event_ms(fn, warmup=1, reps=3):
    """Milliseconds per call of fn() from HIP events around `reps` calls, after `warmup` calls; (mean, min, max)."""
    import torch as t
    for _ in range(warmup):
        fn()
    t.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sum(times) / len(times), min(times), max(times)


def trace_child(path, U, I):
    """The traced work: each stage once per k, on the edges the parent saved."""
    import numpy as np
    import torch as t
    from laplace_amd import ops
    ei = np.load(path).astype(np.int64)
    users, _, csr = device_csr(ei, U, I)
    longest = int(np.diff(users.ptr).max())
    ids, _, sc = ops.cooc_item_neighbors(*csr, T_NEIGHBORS, "cosine")
    for k in KS:
        ops.match_cooccurrence(csr[0], csr[1], ids, sc, k, exclude_seen=True, max_list_len=longest)
        ops.match_common_items(*csr, k)
    t.cuda.synchronize()


def kernel_table(stats_dir):
    f = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        return []
    rows = []
    for r in csv.DictReader(open(f[0])):
        name = r["Name"]
        if "cooc" in name or "match_common" in name:
            m = re.search(r"(\w*(?:cooc|match_common)\w*(?:<[^>]*>)?)", name)
            short = m.group(1) if m else name
            total = float(r.get("TotalDurationNs") or float(r["AverageNs"]) * int(r["Calls"]))
            rows.append((short, int(r["Calls"]), total / 1e6, float(r["AverageNs"]) / 1e6,
                         float(r["MinNs"]) / 1e6, float(r["MaxNs"]) / 1e6))
    return sorted(rows, key=lambda x: -x[2])


def recall_leg(spec, name, eval_users, lightgcn_steps, top_n, popular_n, k_cooc):
    """Candidate recall of the held-out purchases with and without the co-occurrence matcher."""
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, LightGCNMatcher, PopularItemsMatcher
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.run_pipeline_lightgcn import save_predictions
    from laplace_amd.trainer import LightGCNTrainer
    dev = "cuda"
    U, I = spec.num_users, spec.num_items
    t0 = time.perf_counter()
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, eval_users)
    users, articles, _ = device_csr(ei.numpy(), U, I)
    gen_s = time.perf_counter() - t0
    t.manual_seed(0)
    lgcn = LightGCN(U, I, 64, 3).to(dev)
    inter = Interactions(ei.to(dev), U, I)
    trainer = LightGCNTrainer(lgcn, inter.adjacency("bipartite"), inter, lr=0.05, Lambda=1e-6, batch_size=16384, seed=1)
    for _ in range(lightgcn_steps):
        trainer.step()
    trainer.finish()
    top = save_predictions(lgcn, ei.to(dev), num_recommendations=top_n)
    del trainer, inter
    t.cuda.empty_cache()
    hu, hi = held[0].to(dev), held[1].to(dev)
    lg = LightGCNMatcher(top, top_n).matches_for_all_device(U, dev)[hu]
    pop = PopularItemsMatcher.from_adjacency(articles, popular_n).matches_for_all_device(1, dev)[0]
    co = ItemCooccurrenceMatcher(users, articles, k_cooc, neighbors=T_NEIGHBORS, weighting="cosine", exclude_seen=True)
    cooc = co.matches_for_all_device(hu.numel(), dev, query_users=hu)
    in_lg = (lg == hi[:, None]).any(dim=1)
    in_pop = t.isin(hi, pop)
    in_co = (cooc == hi[:, None]).any(dim=1)
    f = lambda m: round(float(m.float().mean()), 4)
    return {"graph": name, "eval_users": int(hu.numel()), "generate_s": round(gen_s, 1), "lightgcn_steps": lightgcn_steps,
            "lightgcn_top": top_n, "popular": popular_n, "cooc_k": k_cooc,
            "recall_lightgcn": f(in_lg), "recall_popular": f(in_pop), "recall_cooc": f(in_co),
            "recall_lightgcn_popular": f(in_lg | in_pop), "recall_lightgcn_popular_cooc": f(in_lg | in_pop | in_co)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cooc_matcher.md"))
    ap.add_argument("--small", action="store_true", help="a 1/50 shape, to rehearse the tool")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--recall", default="c3,planted", help="comma list of c3, planted; empty = none")
    ap.add_argument("--eval-users", type=int, default=20000)
    ap.add_argument("--lightgcn-steps", type=int, default=300)
    ap.add_argument("--trace-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--users", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--items", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child, args.users, args.items)
        return

    import numpy as np
    import torch as t
    from laplace_amd import _lib, ops, synthetic as S
    _lib.lib()
    assert t.cuda.is_available(), "the measurement needs the GPU: there is no CPU path to time"
    spec = S.C3
    planted = S.SyntheticSpec(spec.num_users, spec.num_items, spec.num_edges, seed=2, zipf_s=1.0, communities=32, community_mix=0.9)
    if args.small:
        spec = S.SyntheticSpec(27000, 2100, 640000, seed=2, deg_max=2000, zipf_s=1.0)
        planted = S.SyntheticSpec(27000, 2100, 640000, seed=2, zipf_s=1.0, communities=32, community_mix=0.9)
    U, I = spec.num_users, spec.num_items
    res = {"shape": f"{U} x {I}, {spec.num_edges} edges", "T": T_NEIGHBORS, "device": t.cuda.get_device_name(0)}

    t0 = time.perf_counter()
    ei = S.generate(spec).numpy()
    users, articles, csr = device_csr(ei, U, I)
    res["generate_s"] = round(time.perf_counter() - t0, 1)
    longest = int(np.diff(users.ptr).max())
    deg_i = np.diff(articles.ptr)
    res["longest_user_list"], res["top_item_degree"] = longest, int(deg_i.max())
    res["walks"] = int((np.diff(users.ptr).astype(np.int64) ** 2).sum())   # every list entry of a user x the user's whole list

    table = {}

    def stage1():
        table["t"] = ops.cooc_item_neighbors(*csr, T_NEIGHBORS, "cosine")
    res["stage1_ms"] = [round(x, 2) for x in event_ms(stage1)]
    ids, cnt, sc = table["t"]
    res["stage1_rows_full"] = int((ids[:, -1] >= 0).sum())
    res["stage2_ms"], res["common_items_ms"] = {}, {}
    for k in KS:
        res["stage2_ms"][k] = [round(x, 2) for x in event_ms(
            lambda: ops.match_cooccurrence(csr[0], csr[1], ids, sc, k, exclude_seen=True, max_list_len=longest))]
        res["common_items_ms"][k] = [round(x, 2) for x in event_ms(lambda: ops.match_common_items(*csr, k))]
    res["stage2_workspace_mb"] = round(_lib.lib().mi_match_cooc_workspace_bytes(U, longest, T_NEIGHBORS) / 2 ** 20, 1)
    res["users_beyond_lds"] = int((np.diff(users.ptr) * (T_NEIGHBORS + 1) > 4096).sum())

    kernels = []
    if not args.no_trace:
        tmp = tempfile.mkdtemp(prefix="cooc_trace_")
        try:
            path = os.path.join(tmp, "edges.npy")
            np.save(path, ei.astype(np.int32))
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(tmp, "kt"), "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-child", path, "--users", str(U), "--items", str(I)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the traced run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            kernels = kernel_table(os.path.join(tmp, "kt"))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    del ids, cnt, sc, table, csr
    t.cuda.empty_cache()

    recalls = []
    for name in [x for x in args.recall.split(",") if x]:
        recalls.append(recall_leg({"c3": spec, "planted": planted}[name], name, args.eval_users, args.lightgcn_steps, 100, 50, 100))
    res["recall"] = recalls
    res["kernels"] = [dict(zip(("name", "calls", "total_ms", "avg_ms", "min_ms", "max_ms"), k)) for k in kernels]

    shown = [a for n, a in enumerate(sys.argv[1:], 1) if not a.startswith("--out") and sys.argv[n - 1] != "--out"]   # where it wrote is not part of the recipe
    cmdline = "python tools/bench_cooc.py " + " ".join(shown)
    L = ["# Scored item co-occurrence matcher: measured", "",
         f"Command: `{cmdline.strip()}` on one {res['device']}; {res['shape']} (synthetic.{'C3' if not args.small else 'small'}), "
         f"T = {T_NEIGHBORS}, cosine weighting, exclude_seen.  Longest purchase list {longest}, most popular item held {res['top_item_degree']} times, "
         f"{res['walks']} two-hop walks in the item-side expansion.", "",
         "## Times (HIP events after one warm-up call, 3 calls: mean / min / max, ms)", "",
         "| what | k | ms |", "|---|---|---|",
         f"| stage 1, `mi_cooc_items_topt` (all {I} item rows; {res['stage1_rows_full']} rows have all {T_NEIGHBORS} neighbours) | - | "
         f"{' / '.join(map(str, res['stage1_ms']))} |"]
    for k in KS:
        L.append(f"| stage 2, `mi_match_cooc_i32`, all {U} users | {k} | {' / '.join(map(str, res['stage2_ms'][k]))} |")
    for k in KS:
        L.append(f"| for scale only: `mi_match_common_items_i32` (first k of the walk, no scores), all users | {k} | "
                 f"{' / '.join(map(str, res['common_items_ms'][k]))} |")
    L += ["", f"Stage-2 workspace {res['stage2_workspace_mb']} MiB; {res['users_beyond_lds']} users have more than 4 096 sort slots and take the "
          "workspace path.", ""]
    if kernels:
        L += ["## Kernels (one `rocprofv3 --kernel-trace --stats` run of a child process: stage 1 once, stage 2 and the common-items "
              "matcher once per k)", "", "| kernel | calls | total ms | avg ms | min ms | max ms |", "|---|---|---|---|---|---|"]
        L += [f"| `{n}` | {c} | {tot:.2f} | {avg:.2f} | {mn:.2f} | {mx:.2f} |" for n, c, tot, avg, mn, mx in kernels]
        L.append("")
    if recalls:
        L += ["## Candidate recall of one held-out purchase per user (`synthetic.heldout_edges`)", "",
              "| graph | users | LightGCN top-100 | popular 50 | co-occurrence 100 | [LightGCN, popular] | [LightGCN, popular, co-occurrence] |",
              "|---|---|---|---|---|---|---|"]
        L += [f"| {r['graph']} | {r['eval_users']} | {r['recall_lightgcn']} | {r['recall_popular']} | {r['recall_cooc']} | "
              f"{r['recall_lightgcn_popular']} | {r['recall_lightgcn_popular_cooc']} |" for r in recalls]
        L += ["", f"LightGCN: 3 layers, D = 64, {args.lightgcn_steps} steps of 16 384 (the generator of tools/e2e_hm_scale.py).  `c3` has no planted "
              "structure (nothing to learn beyond popularity); `planted` is the e2e_c3 graph: the same shape with 32 user / item groups.", ""]
    notes = ""   # whatever follows "## Notes" in the file is commentary written by hand: kept
    if os.path.exists(args.out) and "## Notes" in open(args.out).read():
        notes = "## Notes" + open(args.out).read().split("## Notes", 1)[1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + notes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
