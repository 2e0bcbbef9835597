"""The TILES layout of the hub rows (ops.build_hub_tiles_layout, include/laplace_hip.h: mi_spmm_tiles) checked on the host:
torch CPU tensors in, no GPU.  The kernel's summation order is emulated in numpy float32 against float64."""
import numpy as np
import pytest
import torch as t

from laplace_amd import ops

SG, ACC = ops.HUB_SG, ops.HUB_ACC


def _graph(n_cols=3000, seed=0):
    """Item rows over n_cols user columns: one with every column, heavy ones that are cut into 2 and 4 slots, a band of
    medium rows, one whose entries sit in a few tiles only, and short rows that are no hub rows.  Columns 1024..1279 are
    used by no hub row (tiles without a hub entry) apart from the full row, which is left out with dense=False."""
    g = np.random.default_rng(seed)
    rows = []
    rows.append(np.arange(n_cols))                                   # every column
    rows.append(np.sort(g.choice(n_cols, 2400, replace=False)))
    rows.append(np.sort(g.choice(n_cols, 1500, replace=False)))
    for _ in range(40):
        rows.append(np.sort(g.choice(n_cols, int(g.integers(200, 400)), replace=False)))
    rows.append(np.arange(130, 330))                                 # a slot with no entry in most tiles
    for _ in range(30):
        rows.append(np.sort(g.choice(n_cols, int(g.integers(1, 40)), replace=False)))
    return rows


def _csr(rows, n_cols, drop=None, seed=1):
    if drop is not None:
        rows = [r[(r < drop[0]) | (r >= drop[1])] for r in rows]
    g = np.random.default_rng(seed)
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows)
    val = (g.random(col.size) * 0.02 + 0.001).astype(np.float32)
    return ops.DeviceCSR(len(rows), n_cols, t.from_numpy(rowptr.astype(np.int32)), t.from_numpy(col.astype(np.int32)),
                         t.from_numpy(val))


def _layout(a, n_slots=64, floor=150, n_wg=3, tile=64):
    deg = (a.rowptr[1:] - a.rowptr[:-1]).long()
    order = t.argsort(deg, descending=True, stable=True)
    n_hub, parts, bound = ops.hub_tiles_slots(deg[order].tolist(), n_slots, floor)
    hub = order[:n_hub]
    return hub, parts, bound, ops.build_hub_tiles_layout(a, hub, parts, n_wg, tile)


def _entries(lay):
    """Per entry of the layout: (listed tile, sub-group, accumulator), from the counts."""
    cnt = lay["cnt"].numpy().astype(np.int64)
    n_live = cnt.shape[0]
    flat = cnt.reshape(-1)
    ids = np.repeat(np.arange(flat.size), flat)
    return ids // (SG * ACC), (ids // ACC) % SG, ids % ACC, n_live


@pytest.mark.parametrize("n_wg,tile,drop", [(1, 64, None), (3, 64, (1024, 1280)), (8, 128, (1024, 1280)), (300, 64, None)])
def test_every_hub_entry_once_and_in_order(n_wg, tile, drop):
    n_cols = 3000 - 7
    rows = [r[r < n_cols] for r in _graph()]
    if drop is not None:
        rows = rows[1:]                                              # without the full row some tiles hold no hub entry
    a = _csr(rows, n_cols, drop)
    hub, parts, bound, lay = _layout(a, n_wg=n_wg, tile=tile)
    assert len(parts) == hub.numel() and max(parts) >= 2
    src = lay["src"].numpy().astype(np.int64)
    rp = a.rowptr.numpy().astype(np.int64)
    want = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in hub.tolist()])
    assert np.array_equal(np.sort(src), np.sort(want))               # every hub entry exactly once, nothing else
    tj, sg, acc, n_live = _entries(lay)
    assert tj.size == src.size == int(lay["tile_ent"][-1])
    tile_id = lay["tile_id"].numpy().astype(np.int64)
    col = a.col.numpy().astype(np.int64)[src]
    assert np.array_equal(col // tile, tile_id[tj])                  # entries sit in the tile that holds their column
    assert np.array_equal(col % tile, lay["ecol"].numpy().astype(np.int64))
    assert np.array_equal(lay["eval"].numpy(), a.val.numpy()[src])
    # order: (tile, sub-group, accumulator, column), tiles ascending = workgroup-major since the ranges are contiguous
    key = ((tile_id[tj] * SG + sg) * ACC + acc) * (1 << 20) + col
    assert np.all(np.diff(key) > 0)
    # the entry ranges of the tiles and the sub-groups' offsets agree with the counts
    cnt = lay["cnt"].numpy().astype(np.int64)
    assert np.array_equal(np.diff(lay["tile_ent"].numpy()), cnt.sum((1, 2)))
    per_sg = cnt.sum(2)
    assert np.array_equal(lay["sg_off"].numpy(), np.cumsum(per_sg, 1) - per_sg)
    assert lay["max_tile_entries"] == cnt.sum((1, 2)).max()
    if drop is not None:
        assert not np.any((tile_id * tile >= drop[0]) & ((tile_id + 1) * tile <= drop[1]))   # empty tiles are not listed
        assert n_live < (n_cols + tile - 1) // tile
    # one accumulator holds one slot, and a slot is one class of one row
    slot_of = lay["slot_of"].numpy()
    used = slot_of[slot_of >= 0]
    assert np.array_equal(np.sort(used), np.arange(lay["n_slots"])) and lay["n_slots"] == sum(parts)
    row_of_entry = np.searchsorted(rp, src, side="right") - 1
    slot = slot_of[sg * ACC + acc]
    for s in np.unique(slot):
        assert np.unique(row_of_entry[slot == s]).size == 1
    # user ranges: whole tiles, contiguous, covering [0, n_cols)
    cuts = lay["wg_tiles"].numpy()
    n_tiles = (n_cols + tile - 1) // tile
    assert cuts[0] == 0 and cuts[-1] == n_tiles and np.all(np.diff(cuts) >= 0) and cuts.size == n_wg + 1
    wg_ptr = lay["wg_ptr"].numpy()
    assert wg_ptr[0] == 0 and wg_ptr[-1] == n_live
    for w in range(n_wg):
        mine = tile_id[wg_ptr[w]:wg_ptr[w + 1]]
        assert np.all((mine >= cuts[w]) & (mine < cuts[w + 1]))
    if n_wg > n_tiles:
        assert np.sum(np.diff(wg_ptr) == 0) >= n_wg - n_tiles        # idle workgroups
    # item_ptr: n_wg partial rows per slot, hub rows in order
    assert np.array_equal(lay["item_ptr"].numpy(), n_wg * np.concatenate([[0], np.cumsum(parts)]))


def test_no_slot_heavier_than_the_sub_group_mean():
    a = _csr(_graph(), 3000)
    for n_slots in (512, 64, 40):
        hub, parts, bound, lay = _layout(a, n_slots=n_slots)
        deg = (a.rowptr[1:] - a.rowptr[:-1])[hub].tolist()
        assert bound == max(1, sum(deg) // SG)
        assert sum(parts) == lay["n_slots"] <= n_slots
        assert max(lay["slot_loads"]) <= bound
        assert max(parts) >= 4 and min(parts) == 1                   # heavy rows are cut, the others are one slot each
        # longest-processing-time: no sub-group holds more than ACC slots, and the heaviest sub-group is within one slot of the mean
        where = ops.hub_tiles_assign(lay["slot_loads"])
        per = np.zeros(SG)
        for (k, q), ld in zip(where, lay["slot_loads"]):
            assert 0 <= q < ACC
            per[k] += ld
        assert per.max() <= sum(lay["slot_loads"]) / SG + bound


def test_fewer_slots_than_sub_groups_and_exactly_512():
    """The bound of hub_tiles_slots (no slot above total / 32) always yields at least 32 slots, so fewer slots than sub-groups
    exist only for a caller that passes its own parts: the layout must still hold."""
    g = np.random.default_rng(5)
    few = _csr([np.sort(g.choice(2000, 300, replace=False)) for _ in range(5)], 2000)
    lay = ops.build_hub_tiles_layout(few, t.arange(5), [1] * 5, 3, 64)
    assert lay["n_slots"] == 5 and int((lay["slot_of"] >= 0).sum()) == 5
    assert int(lay["tile_ent"][-1]) == 1500
    many = [np.sort(g.choice(2000, 64, replace=False)) for _ in range(600)]
    _, parts, _, lay = _layout(_csr(many, 2000), n_slots=512, floor=64)
    assert lay["n_slots"] == 512 and max(parts) == 1
    assert np.all(lay["slot_of"].numpy() >= 0)


def test_emulated_summation_order_against_float64():
    """Partial row (slot, w) = chained float32 fma over the slot's entries of workgroup w in layout order; a row = the float32
    sum of its partial rows in (slot, w) order.  Bound: the hub-row bound of the full-size test, 1e-5 + 1e-6 sqrt(entries)."""
    n_cols, d, n_wg, tile = 3000, 8, 3, 64
    a = _csr(_graph(), n_cols)
    hub, parts, _, lay = _layout(a, n_wg=n_wg, tile=tile)
    g = np.random.default_rng(3)
    X = (g.standard_normal((n_cols, d)) * 0.1).astype(np.float32)
    tj, sg, acc, _ = _entries(lay)
    slot = lay["slot_of"].numpy()[sg * ACC + acc]
    tile_id = lay["tile_id"].numpy().astype(np.int64)
    col = tile_id[tj] * tile + lay["ecol"].numpy()
    val = lay["eval"].numpy()
    w_of = np.searchsorted(lay["wg_ptr"].numpy(), tj, side="right") - 1
    partial = np.zeros((lay["n_slots"], n_wg, d), dtype=np.float32)
    for i in range(col.size):                                        # layout order = the kernel's order within (slot, w)
        p = partial[slot[i], w_of[i]]
        p[:] = (val[i].astype(np.float64) * X[col[i]].astype(np.float64) + p.astype(np.float64)).astype(np.float32)  # fma: one rounding
    base = np.concatenate([[0], np.cumsum(parts)])
    rp = a.rowptr.numpy()
    for i, r in enumerate(hub.tolist()):
        got = np.zeros(d, dtype=np.float32)
        for s in range(base[i], base[i + 1]):
            for w in range(n_wg):
                got = got + partial[s, w]
        b, e = rp[r], rp[r + 1]
        ref = (a.val.numpy()[b:e].astype(np.float64)[:, None] * X[a.col.numpy()[b:e]].astype(np.float64)).sum(0)
        assert np.abs(got - ref).max() <= 1e-5 + 1e-6 * np.sqrt(e - b), r


def test_user_ranges_balance_the_modelled_cost():
    te = t.tensor([0, 0, 900, 10, 0, 3000, 400, 400, 0, 1], dtype=t.int64)
    cuts = ops.hub_tiles_ranges(te, 64, 3).tolist()
    assert cuts[0] == 0 and cuts[-1] == 10 and cuts == sorted(cuts)
    cost = [0 if x == 0 else max(x, ops.HUB_LOAD_COST * 64) for x in te.tolist()]
    per = [sum(cost[cuts[w]:cuts[w + 1]]) for w in range(3)]
    assert max(per) <= sum(cost) / 3 + max(cost)                     # no range exceeds its share by more than one tile


def test_src_names_the_value_of_every_layout_entry():
    """The layout keeps src (position in val of every layout entry) so that a re-weighted adjacency is one gather into eval.
    Checked here: gathering new values through src gives the eval of a layout built from them.  The re-copy itself
    (ops._sync_plan_values) runs on the device: tests/test_gpu_spmm_hub_tiles.py."""
    a = _csr(_graph(), 3000)
    _, _, _, lay = _layout(a)
    new_val = a.val * 3 + 0.5
    again = lay["eval"].clone()
    again.copy_(new_val[lay["src"].long()])
    a.val = new_val
    _, _, _, lay2 = _layout(a)
    assert t.equal(again, lay2["eval"]) and t.equal(lay["src"], lay2["src"]) and not t.equal(lay["eval"], lay2["eval"])
