"""Host-side premise check for the whole-row path of thin split rows (profiles/thin_rows_c4.md, step 0).

For the item rows of a synthetic graph under the trainer's locality order: rows, entries and banded work items
(band columns per band, chunk entries per work item at most) per degree class.  numpy only, no GPU.

    python tools/thin_rows_table.py [--config c4|c2] [--band 16384] [--chunk 256]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from laplace_amd import synthetic as S  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("c2", "c4"), default="c4")
    ap.add_argument("--band", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=256)
    args = ap.parse_args()
    if args.config == "c4":
        spec = S.C4
        ei = S.generate_blocks(spec, S.C4_BLOCKS, 0, S.C4_BLOCKS, workers=8).numpy()
    else:
        spec = S.C2
        ei = S.generate(spec).numpy()
    u, i = ei[0], ei[1]
    U, I = spec.num_users, spec.num_items
    # interactions.LocalityOrder: items by popularity (stable), users by their coldest item (stable)
    ideg = np.bincount(i, minlength=I)
    item_old_of_new = np.argsort(-ideg, kind="stable")
    item_new_of_old = np.empty(I, dtype=np.int64)
    item_new_of_old[item_old_of_new] = np.arange(I)
    inew = item_new_of_old[i]
    cold = np.zeros(U, dtype=np.int64)
    np.maximum.at(cold, u, inew)
    user_old_of_new = np.argsort(cold, kind="stable")
    user_new_of_old = np.empty(U, dtype=np.int64)
    user_new_of_old[user_old_of_new] = np.arange(U)
    unew = user_new_of_old[u]
    n_bands = -(-U // args.band)
    key = inew * n_bands + unew // args.band          # (item row, band)
    del u, i, ei, unew
    key.sort()
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    starts = np.nonzero(first)[0]
    cnt = np.diff(np.append(starts, key.size))        # entries of every (row, band) pair
    row_of = key[starts] // n_bands
    items_of_row = np.bincount(row_of, weights=-(-cnt // args.chunk), minlength=I).astype(np.int64)
    deg = ideg[item_old_of_new]
    split = deg > args.chunk
    tot_items = int(items_of_row[split].sum())
    print(f"{args.config}: {U} users x {I} items, {key.size} edges; band {args.band} ({n_bands} bands), chunk {args.chunk}")
    print(f"split rows {int(split.sum())}, their entries {int(deg[split].sum())}, work items {tot_items}\n")
    print("| degree | rows | entries | work items | entries / work item | share of work items |")
    print("|---|---|---|---|---|---|")
    edges = [args.chunk, 512, 1024, 2048, 4096, 8192, 1 << 40]
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (deg > lo) & (deg <= hi)
        r, e, w = int(m.sum()), int(deg[m].sum()), int(items_of_row[m].sum())
        name = f"{lo + 1}-{hi}" if hi < (1 << 40) else f"> {lo}"
        print(f"| {name} | {r} | {e} | {w} | {e / max(w, 1):.2f} | {100.0 * w / max(tot_items, 1):.1f} % |")


if __name__ == "__main__":
    main()
