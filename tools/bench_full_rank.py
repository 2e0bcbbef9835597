#!/usr/bin/env python3
"""Time of ops.rank_of_items (csrc/rank.hip) beside its yardstick, top-K on the same rows (profiles/full_rank.md).

  python tools/bench_full_rank.py calls [--rows 16384] [--items 100000] [--dims 128,64,16] [--reps 11] [--excl 10]
      per width: rank_of_items without and with ~`excl` exclusions per row, topk_excl(k = 12) on the same rows and exclusions
      with LAPLACE_TOPK_PREFILTER=0 (the f32 fused kernel: like for like) and with the default.  The legs take turns inside
      every repetition; device events around each call; median, min and max over the repetitions after two warm-up rounds.
      Also the arithmetic of the score sweep (2 rows items d) over the median, as a share of the f32 matrix peak.
  python tools/bench_full_rank.py metrics
      one get_full_rank_metrics_lightgcn call on the planted C1-scale graph of the objective tests (943 x 1682, 100 000 edges,
      8 groups, p = 0.85; 20 000 held-out edges; D 64, K 2, 200 bpr steps), with bench.map_at_12's figure of the same model.
One JSON line per leg."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157.3e12   # MI355X, f32 MFMA (the figure profiles/inbatch_softmax.md uses)


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def calls():
    import torch as t
    from laplace_amd import ops
    dev = "cuda"
    n_q, n_items, reps, per_row = _arg("--rows", 16384), _arg("--items", 100_000), _arg("--reps", 11), _arg("--excl", 10)
    dims = tuple(int(x) for x in _arg("--dims", "128,64,16", str).split(","))
    g = t.Generator(device=dev).manual_seed(0)
    for d in dims:
        ue = t.randn(n_q, d, device=dev, generator=g) * 0.1
        ie = t.randn(n_items, d, device=dev, generator=g) * 0.1
        uid = t.arange(n_q, device=dev)
        target = t.randint(0, n_items, (n_q,), device=dev, generator=g)
        rowptr = (t.arange(n_q + 1, device=dev) * per_row).to(t.int32)
        col = t.randint(0, n_items, (n_q * per_row,), device=dev, generator=g).to(t.int32)
        excl = ops.DeviceCSR(n_q, n_items, rowptr, col)

        def topk(prefilter):
            os.environ["LAPLACE_TOPK_PREFILTER"] = prefilter
            return ops.topk_excl(uid, ue, ie, 12, excl)
        legs = {"rank_of_items": lambda: ops.rank_of_items(uid, target, ue, ie),
                f"rank_of_items, {per_row} exclusions per row": lambda: ops.rank_of_items(uid, target, ue, ie, excl, want_n_excluded=True),
                "topk_excl k=12, f32 fused kernel (LAPLACE_TOPK_PREFILTER=0)": lambda: topk("0"),
                "topk_excl k=12, default": lambda: topk("1")}
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
        os.environ.pop("LAPLACE_TOPK_PREFILTER", None)
        # what was timed is right: the rank of every top-12 entry of the first 256 rows is its column
        top = ops.topk_excl(uid[:256], ue, ie, 12, ops.row_slice(excl, 0, 256))
        rows = t.arange(256, device=dev).repeat_interleave(12)
        ex12 = ops.DeviceCSR(256 * 12, n_items, (t.arange(256 * 12 + 1, device=dev) * per_row).to(t.int32),
                             col[:256 * per_row].view(256, per_row).repeat_interleave(12, dim=0).reshape(-1).contiguous())
        rk = ops.rank_of_items(rows, top.reshape(-1).contiguous(), ue, ie, ex12)
        agree = bool(t.equal(rk.view(256, 12).to(t.int64), t.arange(12, device=dev).expand(256, 12)))
        for name, v in ms.items():
            med = statistics.median(v)
            print(json.dumps({"leg": name, "rows": n_q, "items": n_items, "d": d, "path": ops.rank_path(ue, ie) if "rank" in name else None,
                              "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "reps": len(v),
                              "rows_per_s": round(n_q / (med * 1e-3)),
                              "score_tflops": round(2.0 * n_q * n_items * d / (med * 1e-3) / 1e12, 2),
                              "share_of_f32_matrix_peak": round(2.0 * n_q * n_items * d / (med * 1e-3) / F32_MATRIX_PEAK, 4),
                              "rank_equals_topk_column": agree}), flush=True)


def metrics():
    import time
    import torch as t
    import bench
    from laplace_amd import synthetic as S
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn, get_metrics_lightgcn
    dev = "cuda"
    spec = S.SyntheticSpec(num_users=S.C1.num_users, num_items=S.C1.num_items, num_edges=S.C1.num_edges, seed=5,
                           communities=8, community_mix=0.85, deg_min=1, deg_max=S.C1.num_items // 2)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).to(dev)
    inter = Interactions(ei.to(dev), spec.num_users, spec.num_items)
    t.manual_seed(0)
    model = LightGCN(spec.num_users, spec.num_items, 64, 2).to(dev)
    tr = LightGCNTrainer(model, inter.adjacency("bipartite"), inter, lr=1e-2, Lambda=1e-6, batch_size=1024, seed=7, objective="bpr")
    yard = bench.map_at_12(model, tr, inter, held, 200)          # trains, scores, hands the tables back in original order
    ks = (12, 100, spec.num_items)
    times = []
    for rep in range(7):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        full = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], ks)
        t.cuda.synchronize()
        if rep >= 2:
            times.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    get_metrics_lightgcn(model, held, [inter.edge_index], 12)
    t.cuda.synchronize()
    topk_ms = 1e3 * (time.perf_counter() - t0)
    out = {key: v for key, v in full.items() if not isinstance(v, t.Tensor)}
    print(json.dumps({"leg": "get_full_rank_metrics_lightgcn, planted C1-scale graph, layer-0 tables", "held_out_edges": int(held.shape[1]),
                      "ks": ks, "ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
                      "ms_max": round(max(times), 3), "reps": len(times), "get_metrics_lightgcn_k12_ms_one_call": round(topk_ms, 3),
                      "metrics": out, "bench_map_at_12_layer0": yard["value"], "bench_hit_rate_at_12": yard["hit_rate_at_12"]}))


if __name__ == "__main__":
    {"calls": calls, "metrics": metrics}[sys.argv[1] if len(sys.argv) > 1 else "calls"]()
