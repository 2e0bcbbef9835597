"""Host-side premise check for the TILES form of the hub item rows (profiles/hub_tiles_c4.md, step 1).

For the item rows of a synthetic graph under the trainer's locality order, for H = 64 .. 1024 most popular rows and tiles
of T = 64 / 128 consecutive users: the entries the H rows hold, the entries per tile, the entries per workgroup for P
contiguous user ranges (equal user counts against the product's equal-cost cuts), and the largest slot's share of the hub
entries after the rows heavier than a sub-group's mean load are cut.  numpy only, no GPU.

    python tools/hub_rows_table.py [--config c4|c2] [--wgs 256]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from laplace_amd import synthetic as S  # noqa: E402

LOAD_COST, SG = 6, 32   # ops.HUB_LOAD_COST, ops.HUB_SG


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("c2", "c4"), default="c4")
    ap.add_argument("--wgs", type=int, default=256)
    args = ap.parse_args()
    if args.config == "c4":
        spec = S.C4
        ei = S.generate_blocks(spec, S.C4_BLOCKS, 0, S.C4_BLOCKS, workers=8).numpy()
    else:
        spec = S.C2
        ei = S.generate(spec).numpy()
    u, i = ei[0], ei[1]
    U, I, P = spec.num_users, spec.num_items, args.wgs
    # interactions.LocalityOrder: items by popularity (stable), users by their coldest item (stable)
    ideg = np.bincount(i, minlength=I)
    item_old_of_new = np.argsort(-ideg, kind="stable")
    item_new_of_old = np.empty(I, dtype=np.int64)
    item_new_of_old[item_old_of_new] = np.arange(I)
    inew = item_new_of_old[i]
    cold = np.zeros(U, dtype=np.int64)
    np.maximum.at(cold, u, inew)
    user_new_of_old = np.empty(U, dtype=np.int64)
    user_new_of_old[np.argsort(cold, kind="stable")] = np.arange(U)
    unew = user_new_of_old[u]
    del u, i, ei, cold
    deg = ideg[item_old_of_new]
    cum = np.cumsum(deg)
    print(f"{args.config}: {U} users x {I} items, {inew.size} edges, {P} workgroups\n")
    print("| most popular item rows | entries | share | smallest degree | slots | largest slot's share |")
    print("|---|---|---|---|---|---|")
    for H in (64, 128, 256, 512, 768, 1024):
        tot = int(cum[H - 1])
        bound = max(1, tot // SG)
        parts = -(-deg[:H] // bound)
        largest = int(np.max(-(-deg[:H] // parts)))
        print(f"| {H} | {tot / 1e6:.1f} M | {100.0 * tot / inew.size:.1f} % | {int(deg[H - 1])} | {int(parts.sum())} | "
              f"{100.0 * largest / tot:.2f} % (a sub-group's mean: {100.0 / SG:.2f} %) |")
    print("\n| H | T | entries / tile mean | p50 | p99 | max | entries / workgroup, equal users: min - max | equal cost: min - max |")
    print("|---|---|---|---|---|---|---|---|")
    for H in (64, 128, 256, 512, 768, 1024):
        uh = unew[inew < H]
        for T in (64, 128):
            n_t = -(-U // T)
            te = np.bincount(uh // T, minlength=n_t)
            eq = np.add.reduceat(te, (np.arange(P) * n_t) // P)
            cost = np.where(te > 0, np.maximum(te, LOAD_COST * T), 0)
            cc = np.cumsum(cost)
            cuts = np.minimum(np.searchsorted(cc, (np.arange(1, P) * int(cc[-1])) // P) + 1, n_t)
            edges = np.concatenate([[0], cuts, [n_t]])
            ce = np.concatenate([[0], np.cumsum(te)])
            bal = ce[edges[1:]] - ce[edges[:-1]]
            print(f"| {H} | {T} | {te.mean():.0f} | {int(np.percentile(te, 50))} | {int(np.percentile(te, 99))} | {int(te.max())} | "
                  f"{int(eq.min())} - {int(eq.max())} | {int(bal.min())} - {int(bal.max())} |")


if __name__ == "__main__":
    main()
