#!/usr/bin/env python3
"""Times the device sampler and the ranker's training loop with and without attribute relations
(Config.other_edge_types) at the H&M shape of tools/bench_ranker.py (24 users per batch, 2 hops, fan-out 64).

  sampler   ms per batch of the pipelined iterator alone: next(it) followed by a device synchronise
  loop      ms per iteration of the training loop over the autograd path (forward, BCE, backward, fused Adam), the
            sampler running ahead on its side stream; timed in blocks, one synchronise per block

--relations N attaches N relations with exactly one target per article (50 targets each).  --root DIR imports the package
from another checkout (the same script then times a tree that does not know the relations, with --relations 0).
Prints one JSON line: medians with the 10th / 90th percentile and the extremes."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--relations", type=int, default=0)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=50_000)
    ap.add_argument("--edges", type=int, default=4_000_000)
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--label", default="")
    ap.add_argument("--sampler-only", action="store_true", help="stop after the sampler's timing (short profiled runs)")
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    from types import SimpleNamespace
    import numpy as np
    import torch as t
    from laplace_amd import synthetic as S
    from laplace_amd.data.device_sampler import DeviceGraphSampler
    from laplace_amd.model.encoder_decoder import Encoder_Decoder_Model
    from laplace_amd.model.layers import get_SAGEConv_layers, get_linear_layers
    from laplace_amd.utils.get_info import get_feature_info, select_properties

    dev = "cuda"
    graph, users, articles = S.generate_hetero(S.SyntheticSpec(args.users, args.items, args.edges, seed=2, zipf_s=1.0))
    cfg = SimpleNamespace(k=12, num_neighbors=64, n_hop_neighbors=2, positive_edges_ratio=0.5, negative_edges_ratio=3.0, batch_size=24)
    if args.relations:
        rng = np.random.default_rng(5)
        cfg.other_edge_types, cfg.node_types = [], ["customer", "article"]
        for r in range(args.relations):
            key = ("article", f"has_attr{r}", f"attr{r}")
            graph[key[2]].x = t.from_numpy(rng.integers(0, 10, size=(50, 2)))
            graph[key].edge_index = t.from_numpy(np.stack([np.arange(args.items), rng.integers(0, 50, size=args.items)]))
            cfg.other_edge_types.append(key)
            cfg.node_types.append(key[2])
    loader = DeviceGraphSampler(cfg, graph, users, articles, device=dev, seed=0)

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": float(q[0]), "p10_ms": float(q[1]), "p90_ms": float(q[2]), "min_ms": float(min(ms)),
                "max_ms": float(max(ms)), "n": len(ms)}

    # ---- the sampler alone
    it = iter(loader)
    for _ in range(30):
        next(it)
    t.cuda.synchronize()
    ms = []
    for _ in range(args.batches):
        t0 = time.perf_counter()
        batch = next(it)
        t.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    sampler = stats(ms)
    sizes = {nt: int(batch[nt].x.shape[0]) for nt in batch.node_types}
    it.close()
    if args.sampler_only:
        print(json.dumps({"label": args.label, "relations": args.relations, "sampler_per_batch": sampler, "nodes_in_last_batch": sizes}))
        return

    # ---- the training loop over the autograd path
    t.manual_seed(0)
    it = iter(loader)
    first = next(it)
    model = Encoder_Decoder_Model(get_SAGEConv_layers(2, 128, 64, "add"), get_linear_layers(2, 128, 128, 1), get_feature_info(graph),
                                  first.metadata(), True, "sum", True, 0.2, 0.3).to(dev)
    model.initialize_encoder_input_size(first)
    opt = t.optim.Adam(model.parameters(), lr=0.01, fused=True)
    crit = t.nn.BCEWithLogitsLoss()
    model.train()
    t.autograd.set_multithreading_enabled(False)

    def step(b):
        x, ei, eli, y = select_properties(b)
        opt.zero_grad()
        loss = crit(model(x, ei, eli).view(-1), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(30):
        loss = step(next(it))
    t.cuda.synchronize()
    ms = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        for _ in range(args.block):
            loss = step(next(it))
        t.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.block)
    it.close()
    print(json.dumps({"label": args.label, "relations": args.relations, "sampler_per_batch": sampler, "loop_per_iteration": stats(ms),
                      "nodes_in_last_batch": sizes, "loss": float(loss)}))


if __name__ == "__main__":
    main()
