"""GPU: THIN rows of a banded split-row plan (ops.build_spmm_plan(thin_max=), csrc/spmm.hip spmm_thin_kernel).

Rows with chunk < degree <= thin_max get no work items and no partial rows: a wavefront sums each of them whole, the row's
equal consecutive pieces added in sub-group order.  Every launch form against float64 on the host at the tolerance
tests/test_gpu_lightgcn.py uses for a planned product (1e-6 * sum |val * x| + 1e-6, every width); thin_max = 0 is the plan
and product of before, bit for bit; bitwise reproducible, one stream = two streams, the rare-live hint changes no bit; and
the plan's accounting."""
import pytest
import torch as t

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK, BAND, THIN_MAX = 256, 16384, 1200
N_ROWS, N_COLS = 3000, 140_000                       # 9 bands of 16 384 columns: wide enough for the banded default
# rows on both sides of both thresholds: 256 is short, 257 .. 1200 thin, 1201 and more split
DEGS = {5: 6000, 17: 2600, 40: 1201, 41: 1200, 300: 1199, 999: 900, 1000: 513, 1500: 300, 2998: 257, 2999: 256, 7: 255}
THIN = sorted(r for r, L in DEGS.items() if CHUNK < L <= THIN_MAX)
SPLIT = sorted(r for r, L in DEGS.items() if L > THIN_MAX)


def _ops():
    from laplace_amd import ops
    return ops


@pytest.fixture(scope="module")
def graph():
    ops = _ops()
    g = t.Generator().manual_seed(42)
    rows, cols = [], []
    for r, L in DEGS.items():                        # distinct columns, so that the degrees are exact
        rows.append(t.full((L,), r))
        cols.append(t.randperm(N_COLS, generator=g)[:L])
    free = t.tensor([r for r in range(N_ROWS) if r not in DEGS])
    rows.append(free[t.randint(0, free.numel(), (30000,), generator=g)])
    cols.append(t.randint(0, N_COLS, (30000,), generator=g))
    row, col = t.cat(rows), t.cat(cols)
    key = t.unique(row * N_COLS + col)               # the short rows' duplicates removed
    row, col = key // N_COLS, key % N_COLS
    a = ops.coo_to_csr(row.to(DEV), col.to(DEV), N_ROWS, N_COLS, want_perm=False)
    a.val = (t.rand(a.nnz, generator=g) + 0.5).to(DEV)
    deg = (a.rowptr[1:] - a.rowptr[:-1]).cpu()
    for r, L in DEGS.items():
        assert int(deg[r]) == L
    assert int(deg.max()) == 6000 and int((deg > CHUNK).sum()) == len(THIN) + len(SPLIT)
    return a


def _plans(a):
    ops = _ops()
    thin = ops.build_spmm_plan(a, chunk=CHUNK, band=BAND, thin_max=THIN_MAX)
    zero = ops.build_spmm_plan(a, chunk=CHUNK, band=BAND, thin_max=0)
    return thin, zero


def _f64(a, X):
    """(A X, |A| |X|) in float64 on the host."""
    rp, cc, vv = a.rowptr.cpu().long(), a.col.cpu().long(), a.val.cpu().double()
    rows = t.repeat_interleave(t.arange(a.n_rows), rp[1:] - rp[:-1])
    Xd = X.cpu().double()
    prod = vv[:, None] * Xd[cc]
    want = t.zeros(a.n_rows, X.shape[1], dtype=t.float64).index_add_(0, rows, prod)
    mag = t.zeros(a.n_rows, X.shape[1], dtype=t.float64).index_add_(0, rows, prod.abs())
    return want, mag.max(dim=1).values


def _check(got, want, mag, what, rows=None):
    """Every row within the planned product's tolerance of tests/test_gpu_lightgcn.py: 1e-6 * sum |val * x| + 1e-6."""
    err = (got.cpu().double() - want).abs().max(dim=1).values
    tol = 1e-6 * mag + 1e-6
    if rows is not None:
        err, tol = err[rows], tol[rows]
    worst = int((err - tol).argmax())
    print(f"{what}: max err {float(err.max()):.3e}, smallest tolerance {float(tol.min()):.3e}")
    assert bool((err <= tol).all()), (what, worst, float(err[worst]), float(tol[worst]))


def test_plan_accounting(graph):
    a = graph
    thin, zero = _plans(a)
    deg = (a.rowptr[1:] - a.rowptr[:-1]).cpu()
    assert thin.thin_max == THIN_MAX and zero.thin_max == 0 and zero.thin_rows is None
    # thin + split + short = all rows
    assert thin.n_thin_rows == len(THIN) and thin.n_split_rows == len(SPLIT)
    n_short = int((deg <= CHUNK).sum())
    assert thin.n_thin_rows + thin.n_split_rows + n_short == a.n_rows
    assert thin.n_long_rows == zero.n_long_rows == zero.n_split_rows == len(THIN) + len(SPLIT)
    # the list: exactly the thin rows, longest first
    lst = thin.thin_rows.cpu().long()
    assert sorted(lst.tolist()) == THIN
    dl = deg[lst]
    assert bool((dl[:-1] >= dl[1:]).all())
    assert sorted(thin.long_rows[:thin.n_split_rows].cpu().tolist()) == SPLIT
    # no work item and no partial-row slot belongs to a thin row; every slot belongs to a split row
    items = thin.items.view(-1, 4).cpu()
    real = items[:, 3] >= 0
    assert int(real.sum()) == thin.n_items and set(items[real, 0].tolist()) == set(SPLIT)
    assert sorted(items[real, 3].tolist()) == list(range(thin.n_items))
    ip = thin.item_ptr.cpu()
    assert int(ip[0]) == 0 and int(ip[thin.n_split_rows]) == thin.n_items
    zitems = zero.items.view(-1, 4).cpu()
    n_thin_items = int(((zitems[:, 3] >= 0) & t.isin(zitems[:, 0], t.tensor(THIN))).sum())
    assert n_thin_items > 0 and thin.n_items == zero.n_items - n_thin_items
    # long_index: split rows by position, thin rows -2, short rows -1
    li = thin.long_index.cpu()
    assert bool((li[lst] == -2).all()) and bool((li[t.tensor(SPLIT)] >= 0).all())
    assert int((li == -1).sum()) == n_short


def test_default_rule_gives_thin_rows_only_to_the_banded_default(graph, monkeypatch):
    ops = _ops()
    a = graph
    n_bands = (N_COLS + 1024 - 1) // 1024
    monkeypatch.setattr(ops, "DEFAULT_BAND", 1024)
    monkeypatch.setattr(ops, "THIN_PER_BAND", 4)
    monkeypatch.setattr(ops, "SWEEP", False)
    p = ops.build_spmm_plan(a, chunk=CHUNK)
    assert int(p.struct.band) == 1024 and p.thin_max == 4 * n_bands and p.n_thin_rows == int(sum(CHUNK < L <= 4 * n_bands for L in DEGS.values()))
    monkeypatch.setattr(ops, "THIN_PER_BAND", 0)
    assert ops.build_spmm_plan(a, chunk=CHUNK).n_thin_rows == 0
    monkeypatch.setattr(ops, "THIN_PER_BAND", 4)
    for band in (0, 1024, BAND):                      # a plan whose band is given keeps every long row split
        q = ops.build_spmm_plan(a, chunk=CHUNK, band=band)
        assert q.n_thin_rows == 0 and q.thin_max == 0 and q.n_split_rows == len(THIN) + len(SPLIT)


def test_thin_max_zero_is_the_plan_and_product_of_before(graph):
    """thin_max = 0 against the plan no keyword asks for (what every caller that names a band gets)."""
    ops = _ops()
    a = graph
    _, zero = _plans(a)
    plain = ops.build_spmm_plan(a, chunk=CHUNK, band=BAND)
    for f in ("chunk", "n_long_rows", "n_items", "n_launch", "band", "n_bands"):
        assert getattr(zero.struct, f) == getattr(plain.struct, f), f
    for x, y in ((zero.long_rows, plain.long_rows), (zero.item_ptr, plain.item_ptr), (zero.items, plain.items),
                 (zero.long_index, plain.long_index)) + tuple(zip(zero.packed, plain.packed)):
        assert t.equal(x, y)
    g = t.Generator().manual_seed(1)
    X = t.randn(N_COLS, 128, generator=g).to(DEV)
    outs = []
    for plan in (zero, plain):
        a.plan = plan
        Y = t.full((N_ROWS, 128), float("nan"), device=DEV)
        ops.spmm(a, X, Y=Y)
        outs.append(Y)
    a.plan = None
    assert t.equal(outs[0], outs[1])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_launch_form_against_float64(graph, d):
    ops = _ops()
    a = graph
    thin, _ = _plans(a)
    a.plan = thin
    try:
        g = t.Generator().manual_seed(d)
        X = t.randn(N_COLS, d, generator=g).to(DEV)
        A = t.randn(N_ROWS, d, generator=g).to(DEV)
        want, mag = _f64(a, X)
        # dense: Y, S = scale * (addend + acc)
        Y, S = t.full((N_ROWS, d), float("nan"), device=DEV), t.full((N_ROWS, d), float("nan"), device=DEV)
        ops.spmm(a, X, Y=Y, addend=A, S=S, scale=0.25)
        _check(Y, want, mag, f"dense Y d={d}")
        _check(S, 0.25 * (A.cpu().double() + want), mag, f"dense S d={d}")
        # addend_map: a compact addend for a third of the rows, thin and split rows among them
        has = t.rand(N_ROWS, generator=g) < 0.3
        has[t.tensor(THIN[:3] + SPLIT[:2])] = True
        has[t.tensor(THIN[3:])] = False
        amap = t.full((N_ROWS,), -1, dtype=t.int32)
        amap[has] = t.randperm(int(has.sum()), generator=g).to(t.int32)
        Ac = t.randn(int(has.sum()), d, generator=g).to(DEV)
        Ad = t.zeros(N_ROWS, d, dtype=t.float64)
        Ad[has] = Ac.cpu().double()[amap[has].long()]
        S2 = t.full((N_ROWS, d), float("nan"), device=DEV)
        ops.spmm(a, X, addend=Ac, S=S2, addend_map=amap.to(DEV))
        _check(S2, Ad + want, mag, f"addend_map d={d}")
        # x_map: a compact operand, 5 % of the columns live; with and without the rare-live hint
        keep = t.rand(N_COLS, generator=g) < 0.05
        ids = keep.nonzero().view(-1)
        xmap = t.full((N_COLS,), -1, dtype=t.int32)
        xmap[ids] = t.randperm(ids.numel(), generator=g).to(t.int32)
        Xc = t.randn(ids.numel(), d, generator=g).to(DEV)
        Xe = t.zeros(N_COLS, d)
        Xe[ids] = Xc.cpu()[xmap[ids].long()]
        want_m, mag_m = _f64(a, Xe)
        for rare in (False, True):
            Ym = t.full((N_ROWS, d), float("nan"), device=DEV)
            ops.spmm(a, Xc, Y=Ym, x_map=xmap.to(DEV), x_rare=rare)
            _check(Ym, want_m, mag_m, f"x_map rare={rare} d={d}")
        # row_list through long_index: listed thin, split and short rows at their list positions; a device-side count
        rl = t.tensor([THIN[0], 3, SPLIT[0], THIN[-1], 2999, THIN[2], SPLIT[-1], 7, THIN[1], 100], dtype=t.int32)
        Al = t.randn(rl.numel(), d, generator=g).to(DEV)
        Yl, Sl = t.full((rl.numel(), d), float("nan"), device=DEV), t.full((rl.numel(), d), float("nan"), device=DEV)
        ops.spmm(a, X, Y=Yl, addend=Al, S=Sl, row_list=rl.to(DEV))
        _check(Yl, want[rl.long()], mag[rl.long()], f"row_list Y d={d}")
        _check(Sl, Al.cpu().double() + want[rl.long()], mag[rl.long()], f"row_list S d={d}")
        n_dev = t.tensor([6], dtype=t.int32, device=DEV)
        Yn = t.full((rl.numel(), d), 7.0, device=DEV)
        ops.spmm(a, X, Y=Yn, row_list=rl.to(DEV), n_list_dev=n_dev)
        _check(Yn[:6], want[rl[:6].long()], mag[rl[:6].long()], f"row_list + n_list_dev d={d}")
        assert bool((Yn[6:] == 7.0).all())           # a thin row listed behind the device count is not computed
        # x_map and row_list together
        Ylm = t.full((rl.numel(), d), float("nan"), device=DEV)
        ops.spmm(a, Xc, Y=Ylm, x_map=xmap.to(DEV), row_list=rl.to(DEV))
        _check(Ylm, want_m[rl.long()], mag_m[rl.long()], f"x_map + row_list d={d}")
        # Adam epilogue: the gradient S = scale * (addend + acc) consumed in registers = adam_step on the stored S, bit for bit
        p0 = t.randn(N_ROWS, d, generator=g).to(DEV)
        rw = t.rand(N_ROWS, generator=g).to(DEV)
        for reg_w in (None, rw):
            p2, m2, v2 = p0.clone(), t.zeros(N_ROWS, d, device=DEV), t.zeros(N_ROWS, d, device=DEV)
            G = t.full((N_ROWS, d), float("nan"), device=DEV)
            ops.spmm(a, X, addend=A, S=G, scale=0.5, adam=dict(p=p2, m=m2, v=v2, step=3, lr=1e-2, reg_w=reg_w))
            _check(G, 0.5 * (A.cpu().double() + want), mag, f"adam gradient d={d}")
            p1, m1, v1 = p0.clone(), t.zeros(N_ROWS, d, device=DEV), t.zeros(N_ROWS, d, device=DEV)
            ops.adam_step(p1, G, m1, v1, step=3, lr=1e-2, reg_w=reg_w)
            assert t.equal(p2, p1) and t.equal(m2, m1) and t.equal(v2, v1)
            assert not t.equal(p2[t.tensor(THIN, device=DEV)], p0[t.tensor(THIN, device=DEV)])
    finally:
        a.plan = None


@pytest.mark.parametrize("d", [32, 64, 128])
def test_bitwise_repeatable_one_stream_two_streams_and_rare_hint(graph, d):
    ops = _ops()
    a = graph
    thin, _ = _plans(a)
    a.plan = thin
    saved = ops.SPMM_TWO_STREAMS
    try:
        g = t.Generator().manual_seed(100 + d)
        X = t.randn(N_COLS, d, generator=g).to(DEV)
        A = t.randn(N_ROWS, d, generator=g).to(DEV)
        keep = t.rand(N_COLS, generator=g) < 0.02
        xmap = t.where(keep, t.cumsum(keep.int(), 0) - 1, t.full((N_COLS,), -1)).to(t.int32).to(DEV)
        Xc = X[keep.to(DEV)].contiguous()
        out = {}
        for streams in (1, 0, 2, 1):
            ops.SPMM_TWO_STREAMS = streams
            for rep in (0, 1):
                Y, S = t.full((N_ROWS, d), float("nan"), device=DEV), t.full((N_ROWS, d), float("nan"), device=DEV)
                ops.spmm(a, X, Y=Y, addend=A, S=S, scale=0.5)
                Ym = {}
                for rare in (False, True):
                    Ym[rare] = t.full((N_ROWS, d), float("nan"), device=DEV)
                    ops.spmm(a, Xc, Y=Ym[rare], x_map=xmap, x_rare=rare)
                out.setdefault(streams, []).append((Y, S, Ym[False], Ym[True]))
        t.cuda.synchronize()
        ref = out[1][0]
        assert not bool(t.isnan(ref[0]).any()) and not bool(t.isnan(ref[2]).any())
        assert t.equal(ref[2], ref[3])                                     # the hint changes no bit
        for streams, runs in out.items():
            for run in runs:
                for x, y in zip(run, ref):
                    assert t.equal(x, y), streams                          # run to run, and one stream = two streams
    finally:
        ops.SPMM_TWO_STREAMS = saved
        a.plan = None


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("d", [32, 128, 320])
def test_wavefronts_per_row_setting(graph, d, waves, monkeypatch):
    """LAPLACE_SPMM_THIN_WAVES (A/B): 1, 2 or 4 wavefronts share a thin row; another cut into pieces, the same product."""
    ops = _ops()
    a = graph
    thin, _ = _plans(a)
    a.plan = thin
    monkeypatch.setenv("LAPLACE_SPMM_THIN_WAVES", str(waves))
    try:
        g = t.Generator().manual_seed(7 * d + waves)
        X = t.randn(N_COLS, d, generator=g).to(DEV)
        A = t.randn(N_ROWS, d, generator=g).to(DEV)
        want, mag = _f64(a, X)
        S, S2 = t.full((N_ROWS, d), float("nan"), device=DEV), t.full((N_ROWS, d), float("nan"), device=DEV)
        ops.spmm(a, X, addend=A, S=S, scale=0.5)
        ops.spmm(a, X, addend=A, S=S2, scale=0.5)
        _check(S, 0.5 * (A.cpu().double() + want), mag, f"waves={waves} d={d}")
        assert t.equal(S, S2)
    finally:
        a.plan = None
