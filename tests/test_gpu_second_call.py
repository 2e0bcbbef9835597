"""GPU: state that outlives a call.  Every object here is called once, then one of its INPUTS is changed, then it is
called again — the second call must see the change.

A1  SpMM plans hold copies of the split rows' values (a packed plan's eval, a sweep / hybrid plan's val_s, and the same
    inside plan.wide).  After a re-weighting of the adjacency — in place through torch, by replacement, by replacement with
    an alias of equal (data_ptr, _version), through a raw pointer followed by DeviceCSR.invalidate_values() — every launch
    form of every plan kind gives, row for row, the float64 host product of the CURRENT values at the planned product's
    tolerance (tests/test_gpu_thin_rows.py: 1e-6 * sum |val * x| + 1e-6), and is bitwise reproducible.  The test has power:
    on every split or thin row the old and the new float64 products differ by more than 100 tolerances, so a stale copy
    cannot pass.
A2  data.lightgcn_loader.sample_mini_batch after an in-place edit of edge_index.
A3  NativeRankerStep's raw-pointer descriptor after a BatchNorm buffer, an embedding table or an optimizer state tensor
    was replaced, one at a time.
A4  NativeRankerStep's workspace recovery (MI_ERR_WORKSPACE from the validation pass), single process and with the
    data-parallel vote, without a process group.
A5  NativePinSAGEStep's raw-pointer descriptors (the executor's, Adam's list, the projector's) after a gradient, an Adam moment,
    the projector's code matrix or a text column's tokens was replaced, one at a time; its vote when _prepare raises."""
import copy

import pytest
import torch as t

import test_gpu_thin_rows as TR
from test_gpu_thin_rows import _check, _f64

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 256


def _ops():
    from laplace_amd import ops
    return ops


# ---- A1 ------------------------------------------------------------------------------------------------------------------

def _csr(row, col, n_rows, n_cols, g):
    ops = _ops()
    a = ops.coo_to_csr(row.to(DEV), col.to(DEV), n_rows, n_cols, want_perm=False)
    a.val = (t.rand(a.nnz, generator=g) + 0.5).to(DEV)
    return a


@pytest.fixture(scope="module")
def sweep_graph():
    """The graph of test_spmm_sweep_plan_equals_work_item_plan (tests/test_gpu_lightgcn.py)."""
    g = t.Generator().manual_seed(160)
    n = 6000
    hubs = {3: 5000, 10: 2600, 777: 900, 4000: 300, 5999: 257, 17: 256}
    row = t.cat([t.full((L,), r) for r, L in hubs.items()] + [t.randint(0, n, (30000,), generator=g)])
    col = t.randint(0, n, (row.numel(),), generator=g)
    return _csr(row, col, n, n, g)


@pytest.fixture(scope="module")
def hybrid_graph():
    """The graph of test_hybrid_plan_equals_the_banded_plan: more long rows than 8 * 32 row-part accumulators."""
    g = t.Generator().manual_seed(161)
    n = 9000
    degs = t.cat([t.tensor([6000, 4100, 2500]), t.randint(300, 1500, (380,), generator=g)])
    hub_rows = t.randperm(n, generator=g)[: degs.numel()]
    row = t.cat([t.full((int(L),), int(r)) for r, L in zip(hub_rows, degs)] + [t.randint(0, n, (40000,), generator=g)])
    col = t.randint(0, n, (row.numel(),), generator=g)
    return _csr(row, col, n, n, g)


@pytest.fixture(scope="module")
def thin_graph():
    """The graph of tests/test_gpu_thin_rows.py: rows on both sides of the thin and split thresholds, 140 000 columns."""
    g = t.Generator().manual_seed(42)
    rows, cols = [], []
    for r, L in TR.DEGS.items():
        rows.append(t.full((L,), r))
        cols.append(t.randperm(TR.N_COLS, generator=g)[:L])
    free = t.tensor([r for r in range(TR.N_ROWS) if r not in TR.DEGS])
    rows.append(free[t.randint(0, free.numel(), (30000,), generator=g)])
    cols.append(t.randint(0, TR.N_COLS, (30000,), generator=g))
    row, col = t.cat(rows), t.cat(cols)
    key = t.unique(row * TR.N_COLS + col)
    a = _csr(key // TR.N_COLS, key % TR.N_COLS, TR.N_ROWS, TR.N_COLS, g)
    deg = (a.rowptr[1:] - a.rowptr[:-1]).cpu()
    assert all(int(deg[r]) == L for r, L in TR.DEGS.items())
    return a


# kind -> (graph fixture, width of the product)
KINDS = {"sweep": ("sweep_graph", 64), "sweep_wide": ("sweep_graph", 256), "hybrid": ("hybrid_graph", 64),
         "banded_packed": ("sweep_graph", 64), "row_major_packed": ("sweep_graph", 64), "banded_packed_thin": ("thin_graph", 64),
         "auto_on_the_sweep_graph": ("sweep_graph", 64), "auto_on_the_thin_row_graph": ("thin_graph", 64)}
CHANGES = ("in_place", "replaced", "alias_of_equal_pointer_and_version", "raw_pointer_then_invalidate")


def _fresh(base):
    """An adjacency of its own (values, plan, generation) over the fixture's structure; val at _version 0."""
    ops = _ops()
    a = ops.DeviceCSR(base.n_rows, base.n_cols, base.rowptr, base.col, base.val.clone())
    assert a.val._version == 0
    return a


def _give_plan(kind, a, monkeypatch):
    ops = _ops()
    if kind in ("sweep", "sweep_wide"):
        a.plan = ops.build_sweep_plan(a, chunk=CHUNK, band=64, n_streams=32)
        assert a.plan is not None and a.plan.sweep is not None
    elif kind == "hybrid":
        assert ops.build_sweep_plan(a, chunk=CHUNK, band=64, n_streams=32) is None
        a.plan = ops.build_hybrid_plan(a, chunk=CHUNK, band=64, tail_whole=False, sweep_band=64, n_streams=32)
        assert a.plan is not None and a.plan.sweep is not None and a.plan.items is not None
        assert a.plan.n_items > 8 * int(a.plan.sweep.n_slots)           # a hub half AND a banded half
    elif kind in ("banded_packed", "row_major_packed"):
        a.plan = ops.build_spmm_plan(a, chunk=CHUNK, band=64 if kind == "banded_packed" else 0, sweep=False)
        assert len(a.plan.packed) == 3 and a.plan.sweep is None
    elif kind == "banded_packed_thin":
        a.plan = ops.build_spmm_plan(a, chunk=CHUNK, band=TR.BAND, thin_max=TR.THIN_MAX)
        assert len(a.plan.packed) == 3 and a.plan.n_thin_rows == len(TR.THIN) and a.plan.n_split_rows == len(TR.SPLIT)
    else:                                                               # whatever ops.spmm builds by itself
        a.plan = None
        monkeypatch.setattr(ops, "PLAN_MIN_NNZ", 1)


def _check_auto_form(kind, a):
    """The form ops.spmm chose by itself, pinned so that the case cannot drift to another form unnoticed."""
    ops = _ops()
    if not kind.startswith("auto"):
        return
    assert a.plan is not None
    if kind == "auto_on_the_sweep_graph":    # 6 000 columns < SWEEP_MIN_BANDS * SWEEP_BAND and < MIN_BANDED_COLS: row-major, packed
        assert a.n_cols < ops.SWEEP_MIN_BANDS * ops.SWEEP_BAND and a.n_cols < ops.MIN_BANDED_COLS
        assert a.plan.sweep is None and int(a.plan.struct.band) == 0 and len(a.plan.packed) == 3 and a.plan.n_thin_rows == 0
    else:                                    # 140 000 columns >= 64 * 2 048, ten long rows: the sweep form
        assert a.n_cols >= ops.SWEEP_MIN_BANDS * ops.SWEEP_BAND
        assert a.plan.sweep is not None and a.plan.n_long_rows == len(TR.THIN) + len(TR.SPLIT)


class _Inputs:
    """Operands of every launch form, fixed across the two calls."""

    def __init__(self, a, d, seed):
        g = t.Generator().manual_seed(seed)
        n, m = a.n_rows, a.n_cols
        self.d = d
        self.X = t.randn(m, d, generator=g).to(DEV)
        self.A = t.randn(n, d, generator=g).to(DEV)
        keep = t.rand(m, generator=g) < 0.05
        ids = keep.nonzero().view(-1)
        xmap = t.full((m,), -1, dtype=t.int32)
        xmap[ids] = t.randperm(ids.numel(), generator=g).to(t.int32)
        self.xmap = xmap.to(DEV)
        self.Xc = t.randn(ids.numel(), d, generator=g).to(DEV)
        self.Xe = t.zeros(m, d)
        self.Xe[ids] = self.Xc.cpu()[xmap[ids].long()]
        deg = (a.rowptr[1:] - a.rowptr[:-1]).cpu()
        self.long = (deg > CHUNK).nonzero().view(-1)                    # every split or thin row
        assert self.long.numel() >= 5
        by_len = self.long[t.argsort(deg[self.long], descending=True)]
        short = (deg <= CHUNK).nonzero().view(-1)
        pick = [by_len[0], short[3], by_len[-1], by_len[len(by_len) // 2], short[-1], by_len[1], short[0], by_len[-2], short[1]]
        self.rl = t.stack(pick).to(t.int32)
        self.Al = t.randn(self.rl.numel(), d, generator=g).to(DEV)
        self.p0 = t.randn(n, d, generator=g).to(DEV)


def _launch_forms(a, q):
    """Every launch form tests/test_gpu_thin_rows.py runs, on the adjacency as it is now."""
    ops = _ops()
    n, d, nl = a.n_rows, q.d, q.rl.numel()
    nan = lambda r: t.full((r, d), float("nan"), device=DEV)
    out = {}
    out["Y"], out["S"] = nan(n), nan(n)
    ops.spmm(a, q.X, Y=out["Y"], addend=q.A, S=out["S"], scale=0.25)
    out["Y_again"] = nan(n)
    ops.spmm(a, q.X, Y=out["Y_again"])
    for rare in (False, True):
        out[f"Ym{int(rare)}"] = nan(n)
        ops.spmm(a, q.Xc, Y=out[f"Ym{int(rare)}"], x_map=q.xmap, x_rare=rare)
    out["Yl"], out["Sl"] = nan(nl), nan(nl)
    ops.spmm(a, q.X, Y=out["Yl"], addend=q.Al, S=out["Sl"], row_list=q.rl.to(DEV))
    out["Yn"] = t.full((nl, d), 7.0, device=DEV)
    ops.spmm(a, q.X, Y=out["Yn"], row_list=q.rl.to(DEV), n_list_dev=t.tensor([6], dtype=t.int32, device=DEV))
    out["Ylm"] = nan(nl)
    ops.spmm(a, q.Xc, Y=out["Ylm"], x_map=q.xmap, row_list=q.rl.to(DEV))
    p, m, v = q.p0.clone(), t.zeros(n, d, device=DEV), t.zeros(n, d, device=DEV)
    out["G"] = nan(n)
    ops.spmm(a, q.X, addend=q.A, S=out["G"], scale=0.5, adam=dict(p=p, m=m, v=v, step=3, lr=1e-2))
    out["adam"] = (p, m, v)
    return out


def _check_forms(a, q, out, what):
    """Every row of every form against the float64 host product of the CURRENT a.val."""
    ops = _ops()
    want, mag = _f64(a, q.X)
    want_m, mag_m = _f64(a, q.Xe)
    rl = q.rl.long()
    _check(out["Y"], want, mag, f"{what}: dense Y")
    _check(out["S"], 0.25 * (q.A.cpu().double() + want), mag, f"{what}: dense S")
    assert t.equal(out["Y"], out["Y_again"]), what                      # bitwise reproducible, with and without the epilogue
    for rare in (0, 1):
        _check(out[f"Ym{rare}"], want_m, mag_m, f"{what}: x_map rare={rare}")
    assert t.equal(out["Ym0"], out["Ym1"]), what                        # the hint changes no bit
    _check(out["Yl"], want[rl], mag[rl], f"{what}: row_list Y")
    _check(out["Sl"], q.Al.cpu().double() + want[rl], mag[rl], f"{what}: row_list S")
    _check(out["Yn"][:6], want[rl[:6]], mag[rl[:6]], f"{what}: row_list + n_list_dev")
    assert bool((out["Yn"][6:] == 7.0).all()), what
    _check(out["Ylm"], want_m[rl], mag_m[rl], f"{what}: x_map + row_list")
    _check(out["G"], 0.5 * (q.A.cpu().double() + want), mag, f"{what}: adam gradient")
    p1, m1, v1 = q.p0.clone(), t.zeros_like(q.p0), t.zeros_like(q.p0)
    ops.adam_step(p1, out["G"], m1, v1, step=3, lr=1e-2)
    assert all(t.equal(x, y) for x, y in zip(out["adam"], (p1, m1, v1))), what
    return want, mag


def _reweight(change, a, g):
    """Changes the adjacency's values; returns what must stay alive until the next product."""
    ops = _ops()
    w = (t.rand(a.nnz, generator=g) * 1.5 + 0.5).to(DEV)               # per entry, in [0.5, 2]: no stale copy times a constant
    if change == "in_place":
        a.val.mul_(w)
        return None
    if change == "replaced":
        a.val = (a.val * w).contiguous()
        return None
    if change == "alias_of_equal_pointer_and_version":
        old = a.val
        ptr0, ver0 = old.data_ptr(), old._version
        assert ver0 == 0
        try:
            alias = t.from_dlpack(old)
        except Exception:                                               # the same alias without dlpack
            alias = t.empty(0, device=DEV)
            alias.data = old
        old.mul_(w)
        t.cuda.synchronize()
        # the precondition of this case — it fails, it does not skip: a tensor the old (data_ptr, _version) key cannot tell apart
        assert alias is not old and alias.data_ptr() == ptr0 and alias._version == ver0 and old._version != ver0
        a.val = alias
        return old
    assert change == "raw_pointer_then_invalidate"
    # the library's own writer, through a pointer torch does not see: val[i] = src[idx[i]] (mi_gather_f32)
    from laplace_amd import _lib
    ver0 = a.val._version
    idx = t.randperm(a.nnz, generator=g).to(t.int32).to(DEV)
    src = t.empty(a.nnz, device=DEV)
    src[idx.long()] = a.val * w                                         # so that val[i] becomes val[i] * w[i]
    _lib.check(_lib.lib().mi_gather_f32(a.nnz, src.data_ptr(), idx.data_ptr(), a.val.data_ptr(), _lib.current_stream()),
               "mi_gather_f32")
    assert a.val._version == ver0                                       # torch has not seen it
    a.invalidate_values()                                               # ... so the writer says it
    return (src, idx)


@pytest.mark.parametrize("change", CHANGES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_spmm_plan_follows_a_reweighting(kind, change, request, monkeypatch):
    base = request.getfixturevalue(KINDS[kind][0])
    d = KINDS[kind][1]
    a = _fresh(base)
    _give_plan(kind, a, monkeypatch)
    q = _Inputs(a, d, seed=1000 + len(kind))
    g = t.Generator().manual_seed(len(kind) * 31 + len(change))
    # first call: every copy comes into being (plan, packed values, plan.wide, partial-row workspaces, the live-column bits)
    first = _launch_forms(a, q)
    _check_auto_form(kind, a)
    plan = a.plan
    if kind == "sweep_wide":
        assert plan.wide is not None and plan.wide.sweep is None       # the first wide call came BEFORE the re-weighting
        narrow = _Inputs(a, 64, seed=5)
        narrow_first = _launch_forms(a, narrow)                         # ... and so did the first narrow call, on the sweep itself
        _check_forms(a, narrow, narrow_first, f"{kind} / first call, d=64")
    want_old, _ = _check_forms(a, q, first, f"{kind} / first call")
    sweep_ptr = plan.sweep_t[1].data_ptr() if plan.sweep is not None else None
    keep_alive = _reweight(change, a, g)
    second = _launch_forms(a, q)
    assert a.plan is plan                                               # re-weighted, not re-planned
    if sweep_ptr is not None:                                           # refreshed in place: SpmmSweepStruct keeps its pointer
        assert plan.sweep_t[1].data_ptr() == sweep_ptr == int(plan.sweep.val)
    want_new, mag_new = _check_forms(a, q, second, f"{kind} / after {change}")
    # power: a stale copy cannot pass, on any split or thin row
    gap = (want_new - want_old).abs().max(dim=1).values[q.long]
    tol = (1e-6 * mag_new + 1e-6)[q.long]
    assert bool((gap > 100 * tol).all()), (kind, change, float((gap / tol).min()))
    assert not t.equal(second["Y"], first["Y"])
    if kind == "sweep_wide":                                            # both copies follow, each at its own next call
        _check_forms(a, narrow, _launch_forms(a, narrow), f"{kind} / after {change}, d=64")
    third = _launch_forms(a, q)                                         # and a steady state: nothing left to refresh, same bits
    for k in ("Y", "S", "Ym0", "Yl", "G"):
        assert t.equal(third[k], second[k]), (kind, change, k)
    del keep_alive


def test_unchanged_values_cost_no_refresh(sweep_graph, monkeypatch):
    """The steady state stays what it was: with nothing re-weighted, no pack pass and no gather is enqueued; one re-weighting
    costs one of them, once."""
    ops = _ops()
    from laplace_amd import _lib
    a = _fresh(sweep_graph)
    a.plan = ops.build_sweep_plan(a, chunk=CHUNK, band=64, n_streams=32)
    b = _fresh(sweep_graph)
    b.plan = ops.build_spmm_plan(b, chunk=CHUNK, band=64, sweep=False)
    assert len(b.plan.packed) == 3
    X = t.randn(a.n_cols, 64, device=DEV)
    Y = t.empty(a.n_rows, 64, device=DEV)
    for m in (a, b):
        ops.spmm(m, X, Y=Y)
    calls = []
    L, pack = _lib.lib(), ops._pack_plan_entries

    class Spy:                                                          # the library handle, its mi_gather_f32 counted
        def __getattr__(self, name):
            if name == "mi_gather_f32":
                calls.append("gather")
            return getattr(L, name)
    spy = Spy()
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    monkeypatch.setattr(ops, "_pack_plan_entries", lambda *args, **kw: (calls.append("pack"), pack(*args, **kw))[1])
    for _ in range(3):
        for m in (a, b):
            ops.spmm(m, X, Y=Y)
    assert calls == []
    a.val.mul_(2.0)
    b.val = b.val * 2.0
    for _ in range(3):
        for m in (a, b):
            ops.spmm(m, X, Y=Y)
    assert calls == ["gather", "pack"]


# ---- A2 ------------------------------------------------------------------------------------------------------------------

def test_sample_mini_batch_follows_an_in_place_edit_of_edge_index():
    from laplace_amd.data.lightgcn_loader import sample_mini_batch
    g = t.Generator().manual_seed(7)
    U, I, E, B = 300, 200, 4000, 1024
    users = t.randint(0, U, (E,), generator=g)
    items = t.randint(0, I, (E,), generator=g)
    users[0], items[0], items[1] = U - 1, I - 1, 0
    edge_index = t.stack([users, items]).to(DEV)
    pairs = lambda ei: set((ei[0] * I + ei[1]).cpu().tolist())
    old = pairs(edge_index)

    def draw(step):
        u, p, n = (x.cpu() for x in sample_mini_batch(B, edge_index, seed=3, step=step))
        assert u.numel() == p.numel() == n.numel() == B
        assert int(n.min()) >= 0 and int(n.max()) < int(edge_index[1].max())    # the reference's range [0, max item id)
        return set((u * I + p).tolist())
    assert draw(0) <= old
    edge_index[1].copy_(edge_index[1][t.randperm(E, generator=g).to(DEV)])       # same users, same items, other pairs
    now = pairs(edge_index)
    assert int(edge_index[1].max()) == I - 1 and len(old - now) > E // 2
    got = draw(1)
    assert got <= now, f"{len(got - now)} of {len(got)} sampled positives are not edges of the current edge_index"
    assert not (got & (old - now))
    assert draw(1) == got                                                        # and the same draw again


# ---- A3 / A4 -------------------------------------------------------------------------------------------------------------

def _ranker_pair(seed=3):
    """A model with its twin (shared frozen tables), an Adam each, and a list of batches — the set-up of
    test_native_ranker_step_equals_the_fused_step (tests/test_gpu_ranker.py)."""
    import test_gpu_ranker as TRK
    from laplace_amd.utils.get_info import select_properties
    model, loader, _ = TRK._hetero_setup(seed=seed, aggr="add", embedding=True, p_drop=0.0)
    twin = copy.deepcopy(model)
    twin.embedding_layers = model.embedding_layers
    opt_a = t.optim.Adam(model.parameters(), lr=0.01)
    opt_b = t.optim.Adam(twin.parameters(), lr=0.01)
    model.train(); twin.train()
    batches = []
    for step, batch in enumerate(loader):
        if step == 6:
            break
        batches.append(select_properties(batch.to(DEV)))
    return model, twin, opt_a, opt_b, batches


BN = ("encoder_layer_norm_customer", "encoder_layer_norm_article")


def test_native_ranker_descriptor_follows_replaced_buffers():
    from laplace_amd.ranker_native import NativeRankerStep
    from laplace_amd.ranker_step import FusedRankerStep
    from laplace_amd.utils.constants import Constants
    model, twin, opt_a, opt_b, batches = _ranker_pair()
    native, fused = NativeRankerStep(model, opt_a), FusedRankerStep(twin, opt_b)
    bn_c, bn_a = (getattr(model, n) for n in BN)
    some_param = model.encoder.layers[0][next(iter(model.encoder.layers[0].keys()))].lin_l.weight
    retired = []                                                        # the replaced storages stay alive, and poisoned

    def retire(x, value):
        retired.append(x)
        x.fill_(value)

    def replace_running_var():
        old = bn_c.running_var
        bn_c.running_var = old.clone()
        retire(old, 1e6)
        return lambda: bn_c.running_var

    def replace_num_batches_tracked():
        old = bn_a.num_batches_tracked
        bn_a.num_batches_tracked = old.clone()
        retire(old, 1000)
        return lambda: bn_a.num_batches_tracked

    def replace_table():
        tables = model.embedding_layers[Constants.node_item]            # the twin reads the same list
        old = tables[1]
        tables[1] = old.clone()
        retire(old, 0.25)
        return lambda: tables[1]

    def replace_exp_avg():
        st = opt_a.state[some_param]
        old = st["exp_avg"]
        st["exp_avg"] = old.clone()
        retire(old, 1e3)
        return lambda: st["exp_avg"]

    changes = [None, replace_running_var, replace_num_batches_tracked, replace_table, replace_exp_avg, None]
    for step, ((x, ei, eli, y), change) in enumerate(zip(batches, changes)):
        current = change() if change is not None else None
        before = current().clone() if current is not None else None
        la = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
        lb = fused.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
        what = (step, getattr(change, "__name__", None))
        assert la is not None and lb is not None, (what, native.declined)
        assert float(la) == float(lb), what
        gb = dict(twin.named_parameters())
        for n, p in model.named_parameters():
            assert p.grad is not None and t.equal(p.grad, gb[n].grad), (what, n)
        for bn in BN:                                                   # the CURRENT buffers hold the twin's statistics
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert t.equal(getattr(getattr(model, bn), k), getattr(getattr(twin, bn), k)), (what, bn, k)
        assert int(bn_a.num_batches_tracked) == int(bn_c.num_batches_tracked) == step + 1, what
        for (n, p), q in zip(model.named_parameters(), twin.parameters()):
            assert float((p - q).abs().max()) <= 2e-6, (what, n)      # Adam: same update to rounding (the recipe's bound)
            sa, sb = opt_a.state[p], opt_b.state[q]
            assert float(sa["step"]) == float(sb["step"]) == step + 1
            assert t.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-9), (what, n)
            assert t.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-12), (what, n)
        if change in (replace_running_var, replace_num_batches_tracked, replace_exp_avg):
            assert not t.equal(current(), before), what                 # the new buffer is the one that was written
        twin.load_state_dict(model.state_dict())                        # cut the chain at rounding level, as the recipe does
        for (p, q) in zip(model.parameters(), twin.parameters()):
            for k in ("exp_avg", "exp_avg_sq"):
                opt_b.state[q][k].copy_(opt_a.state[p][k])


def _fresh_executor_step(model, opt, batch, iteration):
    from laplace_amd.ranker_native import NativeRankerStep
    ex = NativeRankerStep(model, opt)
    ex.iteration = iteration
    x, ei, eli, y = batch
    loss = ex.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
    assert loss is not None, ex.declined
    return loss


def test_native_ranker_recovers_from_a_short_workspace(monkeypatch):
    """The state a non-monotone workspace need produces: dims remembered from a batch no smaller than this one, a workspace
    that is too short.  Single process: step() recounts.  Data parallel (world size and vote replaced, no process group):
    _prepare recounts BEFORE the vote, the vote is reached once, with True."""
    from laplace_amd.ranker_native import NativeRankerStep
    model, twin, opt_a, opt_b, batches = _ranker_pair(seed=4)
    twin.embedding_layers = {k: [tb.clone() for tb in v] for k, v in model.embedding_layers.items()}   # two independent runs
    native = NativeRankerStep(model, opt_a)
    batch = batches[0]                                                  # the same batch every time: never larger than the one sized
    x, ei, eli, y = batch

    def same_as_fresh(loss, what):
        want = _fresh_executor_step(twin, opt_b, batch, native.iteration - 1)
        assert float(loss) == float(want), what
        gb = dict(twin.named_parameters())
        for n, p in model.named_parameters():
            assert t.equal(p.grad, gb[n].grad), (what, n)
        for p, q in zip(model.parameters(), twin.parameters()):
            assert t.equal(p, q), what                                  # the same executor code on the same operands: the same update

    l0 = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)  # sizes the workspace on this batch
    assert l0 is not None and native._ws_dims is not None and native._ws.numel() > 4096
    same_as_fresh(l0, "sizing step")
    dims = native._ws_dims
    # single process
    native._ws = t.empty(4096, dtype=t.uint8, device=DEV)
    l1 = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
    assert l1 is not None and native.declined is None
    assert native._ws.numel() >= dims[1] and native._ws_dims is None    # recounted, reallocated, the remembered dims dropped
    same_as_fresh(l1, "single process")
    # with the collective vote
    l2 = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)  # remembers dims again
    same_as_fresh(l2, "re-sized")
    assert native._ws_dims is not None
    native._ws = t.empty(4096, dtype=t.uint8, device=DEV)
    votes = []
    monkeypatch.setattr(NativeRankerStep, "_world", lambda self: 2)
    monkeypatch.setattr(NativeRankerStep, "_all_ranks_take_it", lambda self, mine, device: votes.append(mine) or mine)
    l3 = native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
    assert votes == [True]
    assert l3 is not None and native.declined is None and native._ws.numel() >= dims[1]
    monkeypatch.undo()
    same_as_fresh(l3, "with the vote")


def test_native_ranker_votes_no_before_an_exception_leaves_prepare(monkeypatch):
    """A rank whose _prepare raises must answer the vote first: its peers are already on their way into it."""
    from laplace_amd.ranker_native import NativeRankerStep
    model, twin, opt_a, opt_b, batches = _ranker_pair(seed=5)
    native = NativeRankerStep(model, opt_a)
    x, ei, eli, y = batches[0]
    votes = []
    monkeypatch.setattr(NativeRankerStep, "_world", lambda self: 2)
    monkeypatch.setattr(NativeRankerStep, "_all_ranks_take_it", lambda self, mine, device: votes.append(mine) or mine)

    def boom(self):
        raise RuntimeError("descriptor build failed")
    monkeypatch.setattr(NativeRankerStep, "_build", boom)
    with pytest.raises(RuntimeError, match="descriptor build failed"):
        native.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
    assert votes == [False]


# ---- A5 ------------------------------------------------------------------------------------------------------------------

def _pinsage_model(kind):
    from laplace_amd.pinsage.model import PinSAGEModel
    I, H, LAYERS = 800, 16, 2
    t.manual_seed(H + LAYERS)
    if kind == "id_only":
        return PinSAGEModel(I, H, LAYERS).to(DEV)
    from test_gpu_pinsage_text import _features, _text
    feats = _features(I, (7, 132), 3, _text(I, (60,), 13, tuple(range(9))), 9)     # two code columns, 3 floats, one text column
    return PinSAGEModel(I, H, LAYERS, features=feats).to(DEV)


@pytest.mark.parametrize("kind", ["id_only", "id+cat+dense+text"])
def test_native_pinsage_descriptor_follows_replaced_buffers(kind):
    """Six iterations of one long-lived executor (dropout at the model's 0.5: the iteration counter and the seed show too); before
    iterations 1 to 4 one tensor its descriptors point to is replaced, the old storage kept alive and poisoned.  Every iteration
    equals, bit for bit, a FRESH executor's on a twin that got the same replacement."""
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler
    from test_gpu_pinsage_text import _shared_graph
    U, I, B, SEED = 2500, 800, 48, 31
    users, items = _shared_graph()
    smp = PinSAGESampler(users, items, U, I, batch_size=B, random_walk_length=2, num_layers=2, seed=SEED)
    featured = kind != "id_only"
    model = _pinsage_model(kind)
    with t.no_grad():
        model.bias.normal_(0, 0.1)
    twin = copy.deepcopy(model)
    opt, opt_twin = t.optim.Adam(model.parameters(), lr=3e-3), t.optim.Adam(twin.parameters(), lr=3e-3)
    model.train(); twin.train()
    native = NativePinSAGEStep(model, opt, seed=77)
    retired = []                                                        # the replaced storages stay alive, and poisoned

    def retire(x, poison):
        retired.append(x)
        x.copy_(poison(x)) if callable(poison) else x.fill_(poison)

    def drop_gradients(m, o):
        o.zero_grad(set_to_none=True)

    def replace_exp_avg(m, o):
        st = o.state[m.convs[0].Q.weight]
        old = st["exp_avg"]
        st["exp_avg"] = old.clone()
        retire(old, 1e3)

    def replace_bias_exp_avg_sq(m, o):
        st = o.state[m.bias]
        old = st["exp_avg_sq"]
        st["exp_avg_sq"] = old.clone()
        retire(old, 1e3)

    def replace_bias_grad(m, o):
        old = m.bias.grad
        m.bias.grad = t.zeros_like(m.bias)
        retire(old, 1e3)

    def replace_codes(m, o):
        pr = m.projector
        old = pr.x
        pr.x = old.clone()
        cards = t.tensor(pr.cardinalities, device=old.device)
        retire(old, lambda x: (x + 1) % cards)                          # in range, and another code everywhere

    def replace_tokens(m, o):
        pr = m.projector
        old = pr.text_tok_0
        pr.text_tok_0 = old.clone()
        retire(old, 0)

    changes = [None, drop_gradients, replace_exp_avg] + ([replace_codes, replace_tokens] if featured else
                                                         [replace_bias_exp_avg_sq, replace_bias_grad]) + [None]
    for step, change in enumerate(changes):
        what = (kind, step, getattr(change, "__name__", None))
        if change is not None:
            change(model, opt)
            change(twin, opt_twin)
        batch = smp.sample_batch(step)
        iteration = native.iteration
        la = native.step(batch)
        assert la is not None, (what, native.declined)
        fresh = NativePinSAGEStep(twin, opt_twin, seed=77)
        fresh.iteration = iteration
        lb = fresh.step(batch)
        assert lb is not None, (what, fresh.declined)
        assert float(la) == float(lb), what
        for (n, p), q in zip(model.named_parameters(), twin.parameters()):
            assert t.equal(p, q), (what, n)
            sa, sb = opt.state[p], opt_twin.state[q]
            assert t.equal(sa["exp_avg"], sb["exp_avg"]) and t.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (what, n)
            assert float(sa["step"]) == float(sb["step"]) == step + 1, (what, n)
        if featured:                                                    # the table gradients and the scorer bias's: all-zero again
            pr = model.projector
            for p in [model.bias] + [p for p in pr.parameter_list() if p is not pr.weight and p is not pr.bias]:
                assert float(p.grad.abs().max()) == 0.0, what
    assert len(retired) == 6                                            # three replacements each, model and twin
    if featured:     # a copy (or a pickle) of a projector that has cached descriptors starts without them, and binds its own
        assert model.projector._bound is not None
        clone = copy.deepcopy(model)
        assert clone.projector._bound is None and model.projector._bound is not None
        ids = batch["blocks"][0]["src_ids"]
        assert t.equal(clone.projector.project(ids), model.projector.project(ids))
        assert clone.projector._bound is not None and clone.projector._bound is not model.projector._bound


def test_native_pinsage_votes_no_before_an_exception_leaves_prepare(monkeypatch):
    """As the ranker's: a rank whose _prepare raises must answer the vote first."""
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler
    from test_gpu_pinsage_text import _shared_graph
    users, items = _shared_graph()
    smp = PinSAGESampler(users, items, 2500, 800, batch_size=48, random_walk_length=2, num_layers=2, seed=31)
    model = _pinsage_model("id_only")
    model.train()
    native = NativePinSAGEStep(model, t.optim.Adam(model.parameters(), lr=3e-3))
    votes = []
    monkeypatch.setattr(NativePinSAGEStep, "_world", lambda self: 2)
    monkeypatch.setattr(NativePinSAGEStep, "_all_ranks_take_it", lambda self, mine, device: votes.append(mine) or mine)

    def boom(self):
        raise RuntimeError("descriptor build failed")
    monkeypatch.setattr(NativePinSAGEStep, "_build", boom)
    with pytest.raises(RuntimeError, match="descriptor build failed"):
        native.step(smp.sample_batch(0))
    assert votes == [False]
