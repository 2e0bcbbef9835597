"""GPU: the TILES form of the hub rows (mi_spmm_ex.tiles, ops.HUB_TILES; csrc/spmm.hip spmm_hub_tiles_kernel).

[users; items] adjacencies of about 20 000 user columns and a few hundred item rows.  Against float64 the bound is the hub-row
bound of tests/test_gpu_full_size.py, 1e-5 + 1e-6 * sqrt(entries) per row; everything else is bitwise: run to run, one and two
streams, the Adam epilogue against adam_step, the sparse forms against the form switched off."""
import pytest
import torch as t

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_U, CHUNK = 20011, 256          # 312 tiles of 64 and 43 columns, 156 tiles of 128 and 43: no multiple of either tile


def _ops():
    from laplace_amd import ops
    return ops


def _adjacency(item_rows, n_u=N_U, seed=3):
    """Bipartite [users; items] adjacency from the items' user lists; values 1 / sqrt(deg_u deg_i)."""
    ops = _ops()
    n_i = len(item_rows)
    iu = t.cat([t.as_tensor(r, dtype=t.int64) for r in item_rows])
    ii = t.repeat_interleave(t.arange(n_i), t.tensor([len(r) for r in item_rows]))
    row = t.cat([iu, ii + n_u]).to(DEV)
    col = t.cat([ii + n_u, iu]).to(DEV)
    n = n_u + n_i
    a = ops.coo_to_csr(row, col, n, n, want_perm=False)
    deg = (a.rowptr[1:] - a.rowptr[:-1]).float().clamp(min=1)
    rows = t.repeat_interleave(t.arange(n, device=DEV), (a.rowptr[1:] - a.rowptr[:-1]).long())
    a.val = (1.0 / t.sqrt(deg[rows] * deg[a.col.long()])).contiguous()
    a.plan = ops.build_spmm_plan(a, chunk=CHUNK)
    a.hot = ops.hot_item_rows(n_u, n_i)
    return a


def _main_rows(n_u=N_U, seed=11):
    """Item rows: every user; heavy rows (7 000 and 3 000 entries: cut into 4 and 2 slots beside the full row's 10); 60 rows of 2-4 % of the
    users; a row whose entries sit in three tiles; split rows below the hub floor; short rows.  Users 4096..4607 belong to the
    full row only — with it left out (full=False) those tiles hold no hub entry."""
    g = t.Generator().manual_seed(seed)
    free = t.cat([t.arange(0, 4096), t.arange(4608, n_u)])

    def pick(k):
        return free[t.randperm(free.numel(), generator=g)[:k]].sort().values
    rows = [t.arange(n_u), pick(7000), pick(3000), pick(1500)]
    rows += [pick(int(k)) for k in t.randint(400, 800, (60,), generator=g)]
    rows.append(t.arange(130, 530))                                   # a slot with no entry in most tiles
    rows += [pick(int(k)) for k in t.randint(CHUNK + 1, 340, (12,), generator=g)]   # split rows that are no hub rows
    rows += [pick(int(k)) for k in t.randint(1, 200, (100,), generator=g)]
    return rows


@pytest.fixture(scope="module")
def main_graph():
    return _adjacency(_main_rows())


@pytest.fixture(scope="module")
def holes_graph():
    return _adjacency(_main_rows()[1:])                               # without the full row: tiles without any hub entry


_REF = {}


def _f64(a, X, key):
    if key not in _REF:
        rp = a.rowptr.long()
        rows = t.repeat_interleave(t.arange(a.n_rows, device=DEV), rp[1:] - rp[:-1])
        want = t.zeros(a.n_rows, X.shape[1], dtype=t.float64, device=DEV)
        for lo in range(0, a.nnz, 1 << 18):
            hi = min(a.nnz, lo + (1 << 18))
            want.index_add_(0, rows[lo:hi], a.val[lo:hi].double()[:, None] * X.double()[a.col[lo:hi].long()])
        _REF[key] = want
    return _REF[key]


def _x(a, d, seed=5):
    g = t.Generator().manual_seed(seed)
    return (t.randn(a.n_cols, d, generator=g) * 0.1).to(DEV)


def _check(a, got, want, what):
    deg = (a.rowptr[1:] - a.rowptr[:-1]).double()
    err = (got.double() - want).abs().max(dim=1).values
    tol = 1e-5 + 1e-6 * t.sqrt(deg)
    worst = int((err - tol).argmax())
    print(f"{what}: max err {float(err.max()):.3e} (row of {int(deg[worst])} entries: {float(err[worst]):.3e} of {float(tol[worst]):.3e})")
    assert not bool(t.isnan(got).any()), what
    assert bool((err <= tol).all()), (what, worst, float(err[worst]), float(tol[worst]))


def _force(monkeypatch, on=True, wgs=8, tile=64, slots=512, floor=350, nt=1):
    ops = _ops()
    monkeypatch.setattr(ops, "HUB_TILES", "1" if on else "0")
    monkeypatch.setattr(ops, "HUB_WGS", wgs)
    monkeypatch.setattr(ops, "HUB_TILE", tile)
    monkeypatch.setattr(ops, "HUB_SLOTS", slots)
    monkeypatch.setattr(ops, "HUB_FLOOR", floor)
    monkeypatch.setattr(ops, "HUB_NT", nt)


def _fresh(a):
    a.plan_tiles = None
    return a


def _tiles_plan(a, d=128):
    p = _ops()._hub_tiles_plan_for(a, d)
    assert p is not None and p.tiles is not None
    return p


@pytest.mark.parametrize("wgs,tile,d", [(1, 64, 128), (3, 128, 128), (8, 64, 64), (400, 64, 32), (8, 128, 100), (3, 64, 128)])
def test_product_against_float64_every_range_count_tile_and_width(main_graph, holes_graph, wgs, tile, d, monkeypatch):
    for name, a in (("main", main_graph), ("holes", holes_graph)):
        _force(monkeypatch, wgs=wgs, tile=tile)
        _fresh(a)
        X = _x(a, d)
        plan = _tiles_plan(a, d)
        lay = plan.tiles_t
        parts = (lay["item_ptr"][1:] - lay["item_ptr"][:-1]) // wgs
        assert lay["n_wg"] == wgs and lay["tile"] == tile and 2 in parts.tolist() and (4 in parts.tolist() or name == "holes")
        n_tiles = (a.n_cols + tile - 1) // tile
        listed = int(lay["tile_id"].numel())
        if name == "holes":
            assert listed < (N_U + tile - 1) // tile                  # users 4096..4607: not loaded
        assert listed < n_tiles                                       # nor the tiles of the item columns
        if wgs > n_tiles:
            assert int((lay["wg_ptr"][1:] == lay["wg_ptr"][:-1]).sum()) > 0   # idle workgroups
        assert plan.n_items > wgs * lay["n_slots"] and plan.items is not None  # hub rows + work items: one fix-up
        Y = t.full((a.n_rows, d), float("nan"), device=DEV)
        _ops().spmm(a, X, Y=Y)
        _check(a, Y, _f64(a, X, (name, d)), f"{name} P={wgs} T={tile} d={d}")
        Y2 = t.full((a.n_rows, d), float("nan"), device=DEV)
        _ops().spmm(a, X, Y=Y2)
        assert t.equal(Y, Y2)                                         # run to run


def test_a_wider_product_falls_back_to_the_plain_plan(main_graph, monkeypatch):
    a, d = main_graph, 256
    X = _x(a, d)
    _force(monkeypatch, on=False)
    Y0 = t.empty(a.n_rows, d, device=DEV)
    _ops().spmm(_fresh(a), X, Y=Y0)
    _force(monkeypatch)
    assert _ops()._hub_tiles_plan_for(_fresh(a), d) is None
    Y1 = t.empty(a.n_rows, d, device=DEV)
    _ops().spmm(a, X, Y=Y1)
    assert t.equal(Y0, Y1)


def test_exactly_512_slots_and_fewer_slots_than_sub_groups(monkeypatch):
    ops = _ops()
    g = t.Generator().manual_seed(2)
    rows = [t.randperm(N_U, generator=g)[:300 + k].sort().values for k in range(520)]   # distinct degrees: the cut has no tie
    a = _adjacency(rows)
    _force(monkeypatch, wgs=8, tile=64, floor=CHUNK + 1)
    X = _x(a, 128)
    want = _f64(a, X, ("many", 128))
    plan = _tiles_plan(_fresh(a))
    assert plan.tiles_t["n_slots"] == 512 and int((plan.tiles_t["slot_of"] >= 0).sum()) == 512
    Y = t.full((a.n_rows, 128), float("nan"), device=DEV)
    ops.spmm(a, X, Y=Y)
    _check(a, Y, want, "512 slots")
    # the slot bound always yields 32 slots or more; fewer exist for a layout whose rows are not cut: 5 hub rows, 5 slots
    monkeypatch.setattr(ops, "hub_tiles_slots", lambda deg, n_slots=512, floor=0, n_sg=32: (5, [1] * 5, 0))
    monkeypatch.setattr(ops, "HUB_SLOTS", 5)
    plan = _tiles_plan(_fresh(a))
    assert plan.tiles_t["n_slots"] == 5
    Y = t.full((a.n_rows, 128), float("nan"), device=DEV)
    ops.spmm(a, X, Y=Y)
    _check(a, Y, want, "5 slots")


def test_bitwise_for_one_and_two_streams_and_either_load_policy(main_graph, monkeypatch):
    ops = _ops()
    a = main_graph
    X = _x(a, 128)
    outs = []
    for nt in (1, 0):
        _force(monkeypatch, wgs=8, tile=128, nt=nt)
        _fresh(a)
        for streams in (0, 1, 2):
            monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", streams)
            Y = t.full((a.n_rows, 128), float("nan"), device=DEV)
            ops.spmm(a, X, Y=Y)
            outs.append(Y)
    t.cuda.synchronize()
    for y in outs[1:]:
        assert t.equal(outs[0], y)


def test_epilogues(main_graph, monkeypatch):
    ops = _ops()
    a, d = main_graph, 128
    n = a.n_rows
    _force(monkeypatch, wgs=8, tile=128)
    _tiles_plan(_fresh(a))
    X = _x(a, d)
    want = _f64(a, X, ("main", d))
    g = t.Generator().manual_seed(9)
    A = (t.randn(n, d, generator=g) * 0.1).to(DEV)
    S = A.clone()
    Y = t.empty(n, d, device=DEV)
    ops.spmm(a, X, Y=Y, addend=S, S=S, scale=0.25)                     # S aliases addend
    _check(a, Y, want, "Y beside S")
    _check(a, S * 4, A.double() + want, "S = scale (addend + acc), in place")
    has = t.rand(n, generator=g) < 0.5
    has[N_U:] = t.rand(n - N_U, generator=g) < 0.7                    # most hub rows have an addend row, some have none
    amap = t.full((n,), -1, dtype=t.int32)
    amap[has] = t.randperm(int(has.sum()), generator=g).to(t.int32)
    Ac = (t.randn(int(has.sum()), d, generator=g) * 0.1).to(DEV)
    Ad = t.zeros(n, d, dtype=t.float64, device=DEV)
    Ad[has.to(DEV)] = Ac.double()[amap[has].long().to(DEV)]
    S2 = t.empty(n, d, device=DEV)
    ops.spmm(a, X, addend=Ac, S=S2, addend_map=amap.to(DEV))
    _check(a, S2, Ad + want, "addend_map")
    p0 = (t.randn(n, d, generator=g) * 0.1).to(DEV)
    rw = t.rand(n, generator=g).to(DEV)
    for reg_w in (None, rw):
        p, m, v, G = p0.clone(), t.zeros(n, d, device=DEV), t.zeros(n, d, device=DEV), t.empty(n, d, device=DEV)
        ops.spmm(a, X, addend=A, S=G, scale=0.5, adam=dict(p=p, m=m, v=v, step=3, lr=1e-2, reg_w=reg_w))
        G1 = t.empty(n, d, device=DEV)
        ops.spmm(a, X, addend=A, S=G1, scale=0.5)
        assert t.equal(G, G1)
        p1, m1, v1 = p0.clone(), t.zeros(n, d, device=DEV), t.zeros(n, d, device=DEV)
        ops.adam_step(p1, G1, m1, v1, step=3, lr=1e-2, reg_w=reg_w)
        assert t.equal(p, p1) and t.equal(m, m1) and t.equal(v, v1)
        _check(a, G * 2, A.double() + want, "Adam launch's S")


def test_sparse_forms_keep_todays_plan_bit_for_bit(main_graph, monkeypatch):
    ops = _ops()
    a, d = main_graph, 64
    g = t.Generator().manual_seed(4)
    keep = t.rand(a.n_cols, generator=g) < 0.05
    ids = keep.nonzero().view(-1)
    xmap = t.full((a.n_cols,), -1, dtype=t.int32)
    xmap[ids] = t.randperm(ids.numel(), generator=g).to(t.int32)
    Xc = t.randn(ids.numel(), d, generator=g).to(DEV)
    xmap = xmap.to(DEV)
    rl = t.cat([t.randperm(a.n_rows, generator=g)[:700], t.arange(N_U, N_U + 70)]).to(t.int32).to(DEV)
    X = _x(a, d)

    def run():
        Y = t.empty(a.n_rows, d, device=DEV)
        ops.spmm(a, Xc, Y=Y, x_map=xmap)
        Yr = t.empty(a.n_rows, d, device=DEV)
        ops.spmm(a, Xc, Y=Yr, x_map=xmap, x_rare=True)
        Yl = t.empty(rl.numel(), d, device=DEV)
        ops.spmm(a, X, Y=Yl, row_list=rl)
        return Y, Yr, Yl
    _force(monkeypatch, on=False)
    off = run()
    _force(monkeypatch)
    Yd = t.empty(a.n_rows, d, device=DEV)
    ops.spmm(_fresh(a), X, Y=Yd)                                      # the adjacency now owns a tiles plan
    assert a.plan_tiles is not None and a.plan_tiles is not False
    on = run()
    for x, y in zip(off, on):
        assert t.equal(x, y)
    _check(a, Yd, _f64(a, X, ("main", d)), "dense beside the sparse forms")


def test_reweighting_recopies_the_values(main_graph, monkeypatch):
    ops = _ops()
    a, d = main_graph, 32
    _force(monkeypatch, wgs=3, tile=64)
    X = _x(a, d)
    Y = t.empty(a.n_rows, d, device=DEV)
    ops.spmm(_fresh(a), X, Y=Y)
    old = a.val
    try:
        a.val = old * 2.0
        Y2 = t.empty(a.n_rows, d, device=DEV)
        ops.spmm(a, X, Y=Y2)
        assert t.equal(Y2, Y * 2.0)                                   # a power of two: the same roundings
        a.val.mul_(0.5)                                               # in place: seen through _version
        ops.spmm(a, X, Y=Y2)
        assert t.equal(Y2, Y)
    finally:
        a.val = old
        _fresh(a)
        a.plan = ops.build_spmm_plan(a, chunk=CHUNK)


def _same_thin(x, y):
    return (x is None and y is None) or (x is not None and y is not None and t.equal(x, y))


def test_default_switches_leave_a_small_adjacency_its_plan(main_graph, monkeypatch):
    """The gate: below the column threshold the form does not apply, at the switch's default and at "auto" — no tiles plan, the
    product launched with a.plan (bitwise the form switched off), and the plan spmm() builds for a new adjacency is the one
    build_spmm_plan gives: work items, split rows and thin list."""
    ops = _ops()
    a = main_graph
    X = _x(a, 128)
    monkeypatch.setattr(ops, "HUB_TILES", "0")
    Y0 = t.empty(a.n_rows, 128, device=DEV)
    ops.spmm(_fresh(a), X, Y=Y0)
    monkeypatch.undo()
    for mode in (None, "auto"):
        if mode is not None:
            monkeypatch.setattr(ops, "HUB_TILES", mode)
        if str(ops.HUB_TILES) not in ("auto", "0"):
            continue                                                  # the environment forces the form on: no gate to test
        assert ops._hub_tiles_plan_for(_fresh(a), 128) is None
        Y = t.empty(a.n_rows, 128, device=DEV)
        ops.spmm(a, X, Y=Y)
        assert t.equal(Y, Y0) and not a.plan_tiles and a.plan.tiles is None
        monkeypatch.setattr(ops, "PLAN_MIN_NNZ", 1)
        b = ops.DeviceCSR(a.n_rows, a.n_cols, a.rowptr, a.col, a.val, None, None, a.hot)
        ops.spmm(b, X, Y=Y)                                           # builds b.plan itself
        want = ops.build_spmm_plan(b)
        assert not b.plan_tiles and b.plan.tiles is None
        assert (b.plan.n_items, b.plan.n_long_rows, b.plan.n_split_rows) == (want.n_items, want.n_long_rows, want.n_split_rows)
        assert _same_thin(b.plan.thin_rows, want.thin_rows) and t.equal(b.plan.long_rows, want.long_rows)
        assert t.equal(Y, Y0)


def test_a_refused_lds_size_falls_back_to_the_other_plan(main_graph, monkeypatch):
    """MI_ERR_UNSUPPORTED from a tiles launch (the device refuses the kernel's LDS size): the adjacency gives the form up and
    the product is redone with a.plan — every stream setting, bitwise the form switched off."""
    ops = _ops()
    from laplace_amd import _lib
    a = main_graph
    X = _x(a, 128)
    _force(monkeypatch, on=False)
    Y0 = t.empty(a.n_rows, 128, device=DEV)
    ops.spmm(_fresh(a), X, Y=Y0)
    L = _lib.lib()
    real = L.mi_spmm_csr_ex_f32
    refused = []

    def fake(*args):
        ex = getattr(args[15], "_obj", None)
        if ex is not None and ex.tiles:
            refused.append(1)
            return _lib.MI_ERR_UNSUPPORTED
        return real(*args)
    monkeypatch.setattr(L, "mi_spmm_csr_ex_f32", fake)
    for streams in (1, 0):
        _force(monkeypatch)
        monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", streams)
        _fresh(a)
        refused.clear()
        Y = t.full((a.n_rows, 128), float("nan"), device=DEV)
        ops.spmm(a, X, Y=Y)
        assert len(refused) == 1 and a.plan_tiles is False
        assert t.equal(Y, Y0)
        ops.spmm(a, X, Y=Y)                                           # and stays with a.plan: not tried again
        assert len(refused) == 1 and t.equal(Y, Y0)
    _fresh(a)


def test_trainer_steps_with_the_form_forced_on(monkeypatch):
    """One fused step and ten, form on against form off: the tolerances of test_sparse_batch_step_equals_plain_step."""
    ops = _ops()
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    U, I, E, D, K, B = 4000, 60, 60000, 128, 3, 512
    g = t.Generator().manual_seed(21)
    items = (t.rand(E, generator=g) ** 2 * I).long().clamp(max=I - 1)   # popular items: item rows of up to a few thousand entries
    ei = t.stack([t.randint(0, U, (E,), generator=g), items])
    monkeypatch.setattr(ops, "PLAN_MIN_NNZ", 1)
    tables, losses = {}, {}
    for on in (False, True):
        _force(monkeypatch, on=on, wgs=8, tile=64, floor=300)
        t.manual_seed(21)
        model = LightGCN(U, I, embedding_dim=D, num_iterations=K).to(DEV)
        inter = Interactions(ei, U, I)
        tr = LightGCNTrainer(model, inter.adjacency("bipartite").to(DEV), inter.to(DEV), lr=1e-3, Lambda=1e-4, batch_size=B,
                             seed=9, reorder=True)
        losses[on], tables[on] = [], []
        for it in range(10):
            losses[on].append(float(tr.step()))
            if it in (0, 9):
                tables[on].append(tr.table.clone())
        if on:
            assert tr.adj_fwd.plan_tiles or tr.adj_bwd.plan_tiles       # the form did run
    for la, lb in zip(losses[False], losses[True]):
        assert abs(la - lb) <= 1e-6
    for ta, tb in zip(tables[False], tables[True]):
        assert (ta - tb).abs().max() <= 2e-6
