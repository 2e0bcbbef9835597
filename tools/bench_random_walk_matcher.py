"""Measures the random-walk matcher (csrc/walk_match.hip) at the H&M shape and writes profiles/random_walk_matcher.md:

  * times: mi_match_random_walks_i32 for every user of synthetic.C3 (1 371 980 x 105 542, 31.8 M edges) at the matcher's
    defaults, k = 20 and 100, in milliseconds from HIP events after a warm-up (mean / min / max of three); in the same process,
    as the yardstick, the two stages of the co-occurrence matcher (tools/bench_cooc.py records 117 and 136 ms for them);
  * trace: per-kernel times from ONE `rocprofv3 --kernel-trace --stats` run of a child process of this file (a run of its own:
    tracing slows the host, the event times are taken with the profiler off);
  * recall-c3, recall-planted: the candidate-recall table of profiles/cooc_matcher.md with a "walks 100" column and the unions
    with it, on C3 and on the planted graph of tools/e2e_hm_scale.py.

The parts may run in several calls that share --state (a JSON file of what has been measured so far); the note is rendered from
the whole state every time.

    python tools/bench_random_walk_matcher.py [--parts times,trace,recall-c3,recall-planted] [--state FILE] [--out FILE] [--small]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_cooc as BC   # device_csr, event_ms: one definition of how this family is timed

KS = (20, 100)
DEFAULTS = dict(num_walks=256, walk_length=4, restart_prob=0.5, n_recent=8, boost="multi_hit")   # RandomWalkMatcher's
K_RECALL = 100


def walk_call(csr, ui_sorted, k, **over):
    from laplace_amd import ops
    aptr, aidx, uptr, uidx = csr[2], csr[3], csr[0], csr[1]           # device_csr returns the user lists first
    return ops.match_random_walks(aptr, aidx, uptr, uidx, k, exclude_seen=True, seed=0, ui_sorted=ui_sorted, **dict(DEFAULTS, **over))


def trace_child(path, U, I):
    """The traced work: one call per k, on the edges the parent saved."""
    import numpy as np
    import torch as t
    from laplace_amd import ops
    ei = np.load(path).astype(np.int64)
    _, _, csr = BC.device_csr(ei, U, I)
    ui_sorted = ops.sort_csr_rows(csr[0], csr[1])
    for k in KS:
        walk_call(csr, ui_sorted, k)
    t.cuda.synchronize()


def kernel_table(stats_dir):
    import csv
    import glob
    f = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for r in csv.DictReader(open(f[0])) if f else []:
        if "walk_match" in r["Name"]:
            total = float(r.get("TotalDurationNs") or float(r["AverageNs"]) * int(r["Calls"]))
            rows.append(("walk_match_kernel", int(r["Calls"]), total / 1e6, float(r["AverageNs"]) / 1e6, float(r["MinNs"]) / 1e6,
                         float(r["MaxNs"]) / 1e6))
    return rows


def part_times(spec, res):
    import numpy as np
    import torch as t
    from laplace_amd import ops, synthetic as S
    U, I = spec.num_users, spec.num_items
    t0 = time.perf_counter()
    ei = S.generate(spec).numpy()
    users, articles, csr = BC.device_csr(ei, U, I)
    res["generate_s"] = round(time.perf_counter() - t0, 1)
    res["longest_user_list"] = longest = int(np.diff(users.ptr).max())
    res["sorted_rows_ms"] = [round(x, 2) for x in BC.event_ms(lambda: ops.sort_csr_rows(csr[0], csr[1]))]
    ui_sorted = ops.sort_csr_rows(csr[0], csr[1])
    res["walk_ms"] = {str(k): [round(x, 2) for x in BC.event_ms(lambda: walk_call(csr, ui_sorted, k))] for k in KS}
    res["walk_ms_variants"] = {
        "sum boost": [round(x, 2) for x in BC.event_ms(lambda: walk_call(csr, ui_sorted, 20, boost="sum"))],
        "exclude_seen off": [round(x, 2) for x in BC.event_ms(lambda: ops.match_random_walks(
            csr[2], csr[3], csr[0], csr[1], 20, exclude_seen=False, seed=0, **DEFAULTS))],
        "1024 walks x 4 (the limit), n_recent 16": [round(x, 2) for x in BC.event_ms(
            lambda: walk_call(csr, ui_sorted, 20, num_walks=1024, n_recent=16))],
    }
    _, _, cnt = walk_call(csr, ui_sorted, 20)
    res["mean_distinct_visited"] = round(float(cnt.float().mean()), 1)
    res["users_without_proposal"] = int((cnt == 0).sum())
    table = {}

    def stage1():
        table["t"] = ops.cooc_item_neighbors(*csr, BC.T_NEIGHBORS, "cosine")
    res["cooc_stage1_ms"] = [round(x, 2) for x in BC.event_ms(stage1)]
    ids, _, sc = table["t"]
    res["cooc_stage2_ms"] = {str(k): [round(x, 2) for x in BC.event_ms(
        lambda: ops.match_cooccurrence(csr[0], csr[1], ids, sc, k, exclude_seen=True, max_list_len=longest))] for k in KS}
    return ei


def part_trace(spec, res, ei):
    import numpy as np
    from laplace_amd import synthetic as S
    if ei is None:
        ei = S.generate(spec).numpy()
    tmp = tempfile.mkdtemp(prefix="walk_trace_")
    try:
        path = os.path.join(tmp, "edges.npy")
        np.save(path, ei.astype(np.int32))
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(tmp, "kt"), "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--trace-child", path, "--users", str(spec.num_users),
               "--items", str(spec.num_items)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the traced run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        res["kernels"] = [dict(zip(("name", "calls", "total_ms", "avg_ms", "min_ms", "max_ms"), k))
                          for k in kernel_table(os.path.join(tmp, "kt"))]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def recall_leg(spec, name, eval_users, lightgcn_steps):
    """Candidate recall of the held-out purchases: LightGCN top-100, popular 50, co-occurrence 100, walks 100 and their unions."""
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, LightGCNMatcher, PopularItemsMatcher, RandomWalkMatcher
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.run_pipeline_lightgcn import save_predictions
    from laplace_amd.trainer import LightGCNTrainer
    dev = "cuda"
    U, I = spec.num_users, spec.num_items
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, eval_users)
    users, articles, _ = BC.device_csr(ei.numpy(), U, I)
    t.manual_seed(0)
    lgcn = LightGCN(U, I, 64, 3).to(dev)
    inter = Interactions(ei.to(dev), U, I)
    trainer = LightGCNTrainer(lgcn, inter.adjacency("bipartite"), inter, lr=0.05, Lambda=1e-6, batch_size=16384, seed=1)
    for _ in range(lightgcn_steps):
        trainer.step()
    trainer.finish()
    top = save_predictions(lgcn, ei.to(dev), num_recommendations=100)
    del trainer, inter
    t.cuda.empty_cache()
    hu, hi = held[0].to(dev), held[1].to(dev)
    hit = lambda cand: (cand == hi[:, None]).any(dim=1)
    in_lg = hit(LightGCNMatcher(top, 100).matches_for_all_device(U, dev)[hu])
    in_pop = t.isin(hi, PopularItemsMatcher.from_adjacency(articles, 50).matches_for_all_device(1, dev)[0])
    in_co = hit(ItemCooccurrenceMatcher(users, articles, K_RECALL, neighbors=BC.T_NEIGHBORS, weighting="cosine",
                                        exclude_seen=True).matches_for_all_device(hu.numel(), dev, query_users=hu))
    in_rw = hit(RandomWalkMatcher(users, articles, K_RECALL, exclude_seen=True).matches_for_all_device(hu.numel(), dev, query_users=hu))
    f = lambda m: round(float(m.float().mean()), 4)
    return {"graph": name, "eval_users": int(hu.numel()), "lightgcn_steps": lightgcn_steps,
            "lightgcn": f(in_lg), "popular": f(in_pop), "cooc": f(in_co), "walks": f(in_rw),
            "lightgcn_popular": f(in_lg | in_pop), "lightgcn_popular_cooc": f(in_lg | in_pop | in_co),
            "lightgcn_popular_walks": f(in_lg | in_pop | in_rw), "all_four": f(in_lg | in_pop | in_co | in_rw),
            "walks_only": f(in_rw & ~(in_lg | in_pop | in_co))}


def render(res, out):
    ms = lambda v: " / ".join(map(str, v))
    L = ["# Random-walk matcher: measured", "",
         f"Command: `python tools/bench_random_walk_matcher.py` on one {res.get('device', '?')}; {res.get('shape', '?')}.  Matcher defaults "
         f"({', '.join(f'{k} = {v}' for k, v in DEFAULTS.items())}), exclude_seen, seed 0.", ""]
    if "walk_ms" in res:
        L += ["## Times (HIP events after one warm-up call, 3 calls: mean / min / max, ms)", "", "| what | k | ms |", "|---|---|---|"]
        L += [f"| `mi_match_random_walks_i32`, all users | {k} | {ms(v)} |" for k, v in res["walk_ms"].items()]
        L += [f"| the same, {what} | 20 | {ms(v)} |" for what, v in res["walk_ms_variants"].items()]
        L += [f"| `ops.sort_csr_rows` (the exclusion table, built once per graph) | - | {ms(res['sorted_rows_ms'])} |",
              f"| yardstick, same process: co-occurrence stage 1 `mi_cooc_items_topt` (T = {BC.T_NEIGHBORS}) | - | {ms(res['cooc_stage1_ms'])} |"]
        L += [f"| yardstick, same process: co-occurrence stage 2 `mi_match_cooc_i32`, all users | {k} | {ms(v)} |"
              for k, v in res["cooc_stage2_ms"].items()]
        L += ["", f"Longest purchase list {res['longest_user_list']}; a user's walks visit {res['mean_distinct_visited']} distinct eligible items "
              f"on average; {res['users_without_proposal']} users get no proposal.", ""]
    if res.get("kernels"):
        L += ["## Kernels (one `rocprofv3 --kernel-trace --stats` run of a child process: one call per k)", "",
              "| kernel | calls | total ms | avg ms | min ms | max ms |", "|---|---|---|---|---|---|"]
        L += [f"| `{k['name']}` | {k['calls']} | {k['total_ms']:.2f} | {k['avg_ms']:.2f} | {k['min_ms']:.2f} | {k['max_ms']:.2f} |"
              for k in res["kernels"]]
        L.append("")
    if res.get("recall"):
        L += ["## Candidate recall of one held-out purchase per user (`synthetic.heldout_edges`)", "",
              "| graph | users | LightGCN top-100 | popular 50 | co-occurrence 100 | walks 100 | [LightGCN, popular] | + co-occurrence | + walks | "
              "+ both | found by walks alone |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        L += [f"| {r['graph']} | {r['eval_users']} | {r['lightgcn']} | {r['popular']} | {r['cooc']} | {r['walks']} | {r['lightgcn_popular']} | "
              f"{r['lightgcn_popular_cooc']} | {r['lightgcn_popular_walks']} | {r['all_four']} | {r['walks_only']} |"
              for r in res["recall"].values()]
        L += ["", "LightGCN: 3 layers, D = 64, steps of 16 384 as in tools/bench_cooc.py.  `c3` has no planted structure; `planted` is the "
              "e2e_c3 graph: the same shape with 32 user / item groups.", ""]
    notes = ""   # whatever follows "## Notes" in the file is commentary written by hand: kept
    if os.path.exists(out) and "## Notes" in open(out).read():
        notes = "## Notes" + open(out).read().split("## Notes", 1)[1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(L) + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_walk_matcher.md"))
    ap.add_argument("--parts", default="times,trace,recall-c3,recall-planted")
    ap.add_argument("--state", default=None, help="JSON file shared by calls that run the parts one by one")
    ap.add_argument("--small", action="store_true", help="a 1/50 shape, to rehearse the tool")
    ap.add_argument("--eval-users", type=int, default=20000)
    ap.add_argument("--lightgcn-steps", type=int, default=300)
    ap.add_argument("--trace-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--users", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--items", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child, args.users, args.items)
        return

    import torch as t
    from laplace_amd import _lib, synthetic as S
    _lib.lib()
    assert t.cuda.is_available(), "the measurement needs the GPU: there is no CPU path to time"
    spec = S.C3
    planted = S.SyntheticSpec(spec.num_users, spec.num_items, spec.num_edges, seed=2, zipf_s=1.0, communities=32, community_mix=0.9)
    if args.small:
        spec = S.SyntheticSpec(27000, 2100, 640000, seed=2, deg_max=2000, zipf_s=1.0)
        planted = S.SyntheticSpec(27000, 2100, 640000, seed=2, zipf_s=1.0, communities=32, community_mix=0.9)
    res = json.load(open(args.state)) if args.state and os.path.exists(args.state) else {}
    res["shape"] = f"{spec.num_users} x {spec.num_items}, {spec.num_edges} edges (synthetic.{'small' if args.small else 'C3'})"
    res["device"] = t.cuda.get_device_name(0)
    parts = [p for p in args.parts.split(",") if p]
    say = lambda what: print(f"[bench_random_walk_matcher] {what}", file=sys.stderr, flush=True)
    say(f"parts {parts} on {res['shape']}")
    ei = part_times(spec, res) if "times" in parts else None
    if "trace" in parts:
        say("trace")
        part_trace(spec, res, ei)
    del ei
    t.cuda.empty_cache()
    for name, sp in (("c3", spec), ("planted", planted)):
        if f"recall-{name}" in parts:
            say(f"recall on {name}")
            res.setdefault("recall", {})[name] = recall_leg(sp, name, args.eval_users, args.lightgcn_steps)
    if args.state:
        os.makedirs(os.path.dirname(os.path.abspath(args.state)), exist_ok=True)
        json.dump(res, open(args.state, "w"))
    render(res, args.out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
