"""GPU: the SLICED form of the short-row launch (mi_spmm_ex.row_slices, ops.ROW_SLICES; csrc/spmm.hip spmm_rows_sliced_body).

The workgroup on XCD x computes column slice x % S of a tile of 128 consecutive rows from (col, val) entries staged in LDS
(2 048 per round), rows sorted by length, every output row summed by one sub-group in list order: each launch form must be
torch.equal to the same launch at ROW_SLICES = 0 and within the planned product's tolerance of tests/test_gpu_lightgcn.py
(1e-6 * sum |val * x| + 1e-6) of a float64 product."""
import pytest
import torch as t

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK, TILE, CAP = 256, 128, 2048
N_ROWS, N_COLS = 3001, 9000                          # 23 tiles and 57 rows: not a multiple of the tile, nor of 8 / S tiles
# degree 0, 1, exactly chunk, chunk + 1 and more (the split path; 4 000 entries do not fit one round, 300 lie between short
# rows of one round), and rows 1024 .. 1151 = one whole tile of 40-entry rows: 5 120 entries, two rounds
DEGS = {0: 0, 1: 1, 2: CHUNK, 3: CHUNK + 1, 130: 0, 131: CHUNK, 700: 4000, 1500: 300, 2999: 0, 3000: 17}
DEGS.update({r: 40 for r in range(1024, 1152)})


def _ops():
    from laplace_amd import ops
    return ops


@pytest.fixture(scope="module")
def graph():
    ops = _ops()
    g = t.Generator().manual_seed(7)
    deg = t.exp(t.randn(N_ROWS, generator=g) * 0.9 + 2.2).long().clamp(0, 200)   # lognormal lengths, median 9
    for r, L in DEGS.items():
        deg[r] = L
    rows = t.repeat_interleave(t.arange(N_ROWS), deg)
    cols = t.cat([t.randperm(N_COLS, generator=g)[:int(L)].sort().values for L in deg.tolist()])  # distinct: exact degrees
    a = ops.coo_to_csr(rows.to(DEV), cols.to(DEV), N_ROWS, N_COLS, want_perm=False)
    a.val = (t.rand(a.nnz, generator=g) + 0.5).to(DEV)
    got = (a.rowptr[1:] - a.rowptr[:-1]).cpu()
    assert t.equal(got, deg) and int(a.rowptr[-1]) == a.nnz and int(got[-1]) == 17   # the last row ends at nnz
    assert int(got[1024:1152].sum()) > CAP
    a.plan = ops.build_spmm_plan(a, chunk=CHUNK)
    assert int(a.plan.struct.chunk) == CHUNK and a.plan.n_long_rows == 3
    a.hot = (0, 1)                                   # the hint that marks popularity-ordered columns
    return a


def _f64(a, X):
    """(A X, row-wise max over columns of |A| |X|) in float64."""
    rp = a.rowptr.long()
    rows = t.repeat_interleave(t.arange(a.n_rows, device=DEV), rp[1:] - rp[:-1])
    prod = a.val.double()[:, None] * X.double()[a.col.long()]
    want = t.zeros(a.n_rows, X.shape[1], dtype=t.float64, device=DEV).index_add_(0, rows, prod)
    mag = t.zeros(a.n_rows, X.shape[1], dtype=t.float64, device=DEV).index_add_(0, rows, prod.abs())
    return want, mag.max(dim=1).values


def _check(got, want, mag, what):
    err = (got.double() - want).abs().max(dim=1).values
    tol = 1e-6 * mag + 1e-6
    print(f"{what}: max err {float(err.max()):.3e}, smallest tolerance {float(tol.min()):.3e}")
    worst = int((err - tol).argmax())
    assert bool((err <= tol).all()), (what, worst, float(err[worst]), float(tol[worst]))


def _nan(n, d):
    return t.full((n, d), float("nan"), device=DEV)


def _forms(a, d, seed):
    """Every launch form the sliced kernel serves, as (name, run) with run() -> dict of outputs, and the float64 answers."""
    ops = _ops()
    n = a.n_rows
    g = t.Generator().manual_seed(seed)
    X = t.randn(a.n_cols, d, generator=g).to(DEV)
    A = t.randn(n, d, generator=g).to(DEV)
    want, mag = _f64(a, X)
    forms, answers = {}, {}

    def dense():
        Y, S = _nan(n, d), _nan(n, d)
        ops.spmm(a, X, Y=Y, addend=A, S=S, scale=0.25)
        return {"Y": Y, "S": S}
    forms["dense"], answers["dense"] = dense, {"Y": (want, mag), "S": (0.25 * (A.double() + want), mag)}

    def y_only():
        Y = _nan(n, d)
        ops.spmm(a, X, Y=Y)
        return {"Y": Y}
    forms["y_only"], answers["y_only"] = y_only, {"Y": (want, mag)}

    def s_only():
        S = _nan(n, d)
        ops.spmm(a, X, S=S, scale=2.0)               # no addend
        return {"S": S}
    forms["s_only"], answers["s_only"] = s_only, {"S": (2.0 * want, 2.0 * mag)}

    has = t.rand(n, generator=g) < 0.3
    amap = t.full((n,), -1, dtype=t.int32)
    amap[has] = t.randperm(int(has.sum()), generator=g).to(t.int32)
    Ac = t.randn(int(has.sum()), d, generator=g).to(DEV)
    Ad = t.zeros(n, d, dtype=t.float64, device=DEV)
    Ad[has.to(DEV)] = Ac.double()[amap[has].long().to(DEV)]
    amap = amap.to(DEV)

    def addend_map():
        S = _nan(n, d)
        ops.spmm(a, X, addend=Ac, S=S, addend_map=amap)
        return {"S": S}
    forms["addend_map"], answers["addend_map"] = addend_map, {"S": (Ad + want, mag)}

    for live in (0.0, 0.05, 1.0):
        keep = t.rand(a.n_cols, generator=g) < live
        ids = keep.nonzero().view(-1)
        xmap = t.full((a.n_cols,), -1, dtype=t.int32)
        xmap[ids] = t.randperm(ids.numel(), generator=g).to(t.int32)
        Xc = t.randn(max(ids.numel(), 1), d, generator=g).to(DEV)
        Xe = t.zeros(a.n_cols, d, device=DEV)
        if ids.numel():
            Xe[ids.to(DEV)] = Xc[xmap[ids].long().to(DEV)]
        xmap = xmap.to(DEV)

        def x_map(Xc=Xc, xmap=xmap):
            Y = _nan(n, d)
            ops.spmm(a, Xc, Y=Y, x_map=xmap)
            return {"Y": Y}
        forms[f"x_map_{live}"], answers[f"x_map_{live}"] = x_map, {"Y": _f64(a, Xe)}

    p0 = t.randn(n, d, generator=g).to(DEV)
    rw = t.rand(n, generator=g).to(DEV)
    for name, reg_w in (("adam", None), ("adam_reg_w", rw)):
        def adam(reg_w=reg_w):
            p, m, v, G = p0.clone(), t.zeros(n, d, device=DEV), t.zeros(n, d, device=DEV), _nan(n, d)
            ops.spmm(a, X, addend=A, S=G, scale=0.5, adam=dict(p=p, m=m, v=v, step=3, lr=1e-2, reg_w=reg_w))
            p1, m1, v1 = p0.clone(), t.zeros(n, d, device=DEV), t.zeros(n, d, device=DEV)
            ops.adam_step(p1, G, m1, v1, step=3, lr=1e-2, reg_w=reg_w)   # the epilogue = adam_step after the plain product
            assert t.equal(p, p1) and t.equal(m, m1) and t.equal(v, v1), name
            return {"S": G, "p": p, "m": m, "v": v}
        forms[name], answers[name] = adam, {"S": (0.5 * (A.double() + want), mag)}
    return forms, answers


def _run_all(forms, slices, monkeypatch):
    monkeypatch.setattr(_ops(), "ROW_SLICES", slices)
    monkeypatch.setattr(_ops(), "ROW_SLICES_FORMS", 7)   # every form, not only the ones sliced by default
    monkeypatch.setattr(_ops(), "ROW_SLICES_MIN_REUSE", 0)  # and whatever the graph's size
    out = {name: run() for name, run in forms.items()}
    t.cuda.synchronize()
    return out


@pytest.mark.parametrize("slices", [2, 4])
@pytest.mark.parametrize("d", [128, 64, 32])
def test_every_form_is_bitwise_the_plain_launch_and_close_to_float64(graph, d, slices, monkeypatch):
    forms, answers = _forms(graph, d, seed=1000 + d)
    plain = _run_all(forms, 0, monkeypatch)
    sliced = _run_all(forms, slices, monkeypatch)
    for name, outs in sliced.items():
        for k, got in outs.items():
            assert not bool(t.isnan(got).any()), (name, k)
            assert t.equal(got, plain[name][k]), (name, k)
        for k, (want, mag) in answers[name].items():
            _check(outs[k], want, mag, f"{name} {k} d={d} S={slices}")
            _check(plain[name][k], want, mag, f"{name} {k} d={d} S=0")


@pytest.mark.parametrize("slices", [2, 4])
def test_a_width_without_whole_slices_keeps_the_plain_kernel(graph, slices, monkeypatch):
    forms, _ = _forms(graph, 100, seed=5)            # 25 float4 per row
    plain = _run_all(forms, 0, monkeypatch)
    sliced = _run_all(forms, slices, monkeypatch)
    for name, outs in sliced.items():
        for k, got in outs.items():
            assert t.equal(got, plain[name][k]), (name, k)


@pytest.mark.parametrize("slices", [2, 4])
def test_rows_behind_the_hot_rows_keep_the_plain_kernel(graph, slices, monkeypatch):
    """a.hot = (first hot row, rows): the rows in front of it run sliced, the others plain, in one call (mi_spmm_ex.slice_rows)."""
    a = graph
    forms, answers = _forms(a, 128, seed=11)
    plain = _run_all(forms, 0, monkeypatch)
    try:
        for first in (1, 1100, 1700, N_ROWS):        # inside the first tile, inside the two-round tile, anywhere, all rows
            a.hot = (first, 1)
            sliced = _run_all(forms, slices, monkeypatch)
            for name, outs in sliced.items():
                for k, got in outs.items():
                    assert t.equal(got, plain[name][k]), (first, name, k)
                for k, (want, mag) in answers[name].items():
                    _check(outs[k], want, mag, f"{name} {k} first hot row {first} S={slices}")
    finally:
        a.hot = (0, 1)


def test_one_stream_and_two_streams(graph, monkeypatch):
    ops = _ops()
    forms, _ = _forms(graph, 128, seed=9)
    monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", 1)
    ref = _run_all(forms, 0, monkeypatch)
    for streams in (0, 1, 2):
        monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", streams)
        for slices in (2, 4):
            out = _run_all(forms, slices, monkeypatch)
            for name, outs in out.items():
                for k, got in outs.items():
                    assert t.equal(got, ref[name][k]), (streams, slices, name, k)


def test_streaming_stores_of_outputs_of_64_mb(monkeypatch):
    """Outputs of n_rows * d * 4 >= 64 MB leave through the streaming store path."""
    ops = _ops()
    n, n_cols, d = 131_072 + 77, 20_000, 128
    g = t.Generator().manual_seed(3)
    deg = t.exp(t.randn(n, generator=g) * 0.8 + 1.7).long().clamp(0, 60)
    rows = t.repeat_interleave(t.arange(n), deg)
    cols = t.randint(0, n_cols, (int(deg.sum()),), generator=g)
    a = ops.coo_to_csr(rows.to(DEV), cols.to(DEV), n, n_cols, want_perm=False)
    a.val = (t.rand(a.nnz, generator=g) + 0.5).to(DEV)
    a.plan = ops.build_spmm_plan(a, chunk=CHUNK)
    a.hot = (0, 1)
    assert n * d * 4 >= 64 << 20
    X = t.randn(n_cols, d, generator=g).to(DEV)
    A = t.randn(n, d, generator=g).to(DEV)
    want, mag = _f64(a, X)
    outs = {}
    for slices in (0, 2, 4):
        monkeypatch.setattr(ops, "ROW_SLICES", slices)
        monkeypatch.setattr(ops, "ROW_SLICES_FORMS", 7)
        monkeypatch.setattr(ops, "ROW_SLICES_MIN_REUSE", 0)
        Y, S = _nan(n, d), _nan(n, d)
        ops.spmm(a, X, Y=Y, addend=A, S=S, scale=0.5)
        outs[slices] = (Y, S)
    t.cuda.synchronize()
    for slices in (2, 4):
        assert t.equal(outs[slices][0], outs[0][0]) and t.equal(outs[slices][1], outs[0][1]), slices
        _check(outs[slices][0], want, mag, f"streaming Y S={slices}")
        _check(outs[slices][1], 0.5 * (A.double() + want), mag, f"streaming S S={slices}")
