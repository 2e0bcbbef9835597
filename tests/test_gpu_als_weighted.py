"""GPU: the weighted iALS row solves (mi_als_solve_rows_w_f32, mi_als_block_rows_w_f32) against the float64 statement of their
rules (tests/als_weighted_emulation.py): inside the derived bound, within 8 times the float32 reference's own distance where the
block form has several blocks, constant weights against the UNWEIGHTED rule, two exact cases, equal bits across calls, batches,
row lists and paths, the unweighted ops and the default model untouched, failed rows, and als.ImplicitALS with per-edge
confidences and reg_power end to end."""
import numpy as np
import pytest
import torch as t

import als_block_emulation as BE
import als_emulation as AE
import als_weighted_cases as WC
import als_weighted_emulation as WE
from laplace_amd import _lib, ops
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions

pytestmark = pytest.mark.gpu

N_COLS = WC.N_COLS
F = np.float32


def _dev(a, dtype=None):
    x = t.from_numpy(np.ascontiguousarray(a)).cuda()
    return x if dtype is None else x.to(dtype)


def _csr(rows, conf, n_cols=N_COLS):
    ptr, idx, cf = WC.csr_arrays(rows, conf)
    return ops.DeviceCSR(len(rows), n_cols, _dev(ptr), _dev(idx)), _dev(cf)


class Chol:
    """The device side of one WC.CholProblem and its one batched call."""

    def __init__(self, d):
        self.pr = WC.chol_problem(d)
        self.d = d
        self.Y_dev = _dev(self.pr.wide)[:, 4:4 + d]
        self.G_dev = _dev(self.pr.G)
        self.csr, self.conf_dev = _csr(self.pr.rows, self.pr.conf)
        self.reg_dev = _dev(self.pr.reg_rows)
        X, nf = self.call()
        assert int(nf.item()) == 0
        self.X_dev, self.X = X, X.cpu().numpy()

    def call(self, **kw):
        return ops.als_solve_rows(self.csr, self.Y_dev, self.G_dev, alpha=1.0, reg=1.0, conf=self.conf_dev,
                                  reg_rows=self.reg_dev, **kw)

    def alone(self, r):
        """Row r as its own one-row CSR (reg_rows then has one entry)."""
        csr, cf = _csr([self.pr.rows[r]], [self.pr.conf[r]])
        return ops.als_solve_rows(csr, self.Y_dev, self.G_dev, alpha=1.0, reg=1.0, conf=cf, reg_rows=self.reg_dev[r:r + 1])


class Block:
    """The device side of one WC.BlockProblem; one batched call per start, kept."""

    def __init__(self, d, B):
        self.pr = WC.block_problem(d, B)
        self.d, self.B = d, B
        self.Y_dev = _dev(self.pr.wide)[:, 4:4 + d]
        self.G_dev = _dev(self.pr.G)
        self.X0_dev = _dev(self.pr.X0)
        self.csr, self.conf_dev = _csr(self.pr.rows, self.pr.conf)
        self.reg_dev = _dev(self.pr.reg_rows)
        self._out = {}

    def call(self, from_zero, sweeps, rows=None, row_list=None):
        x = None
        if not from_zero:
            x = self.X0_dev.clone() if rows is None else self.X0_dev[rows].clone()
        return ops.als_block_rows(self.csr, self.Y_dev, self.G_dev, alpha=1.0, reg=1.0, block=self.B, sweeps=sweeps, x=x,
                                  row_list=row_list, conf=self.conf_dev, reg_rows=self.reg_dev)

    def alone(self, r, from_zero, sweeps):
        csr, cf = _csr([self.pr.rows[r]], [self.pr.conf[r]])
        x = None if from_zero else self.X0_dev[r:r + 1].clone()
        return ops.als_block_rows(csr, self.Y_dev, self.G_dev, alpha=1.0, reg=1.0, block=self.B, sweeps=sweeps, x=x, conf=cf,
                                  reg_rows=self.reg_dev[r:r + 1])

    def out(self, from_zero, sweeps):
        if (from_zero, sweeps) not in self._out:
            X, nf = self.call(from_zero, sweeps)
            assert int(nf.item()) == 0
            self._out[(from_zero, sweeps)] = X
        return self._out[(from_zero, sweeps)]


_CASES = {}


def _chol(d):
    if d not in _CASES:
        _CASES[d] = Chol(d)
    return _CASES[d]


def _block(d, B):
    if (d, B) not in _CASES:
        _CASES[(d, B)] = Block(d, B)
    return _CASES[(d, B)]


@pytest.fixture(params=WC.CHOL_DIMS, ids=lambda d: f"d{d}")
def chol(request):
    return _chol(request.param)


@pytest.fixture(params=WC.BLOCK_SHAPES, ids=lambda s: f"d{s[0]}-B{s[1]}")
def block(request):
    return _block(*request.param)


# ---- 1. the Cholesky form inside the derived bound ------------------------------------------------------------------------------
def test_cholesky_batch_inside_the_bound(chol):
    assert chol.Y_dev.stride(0) == chol.d + 8
    for r in range(chol.pr.N_ROWS):
        chol.pr.check_row(r, chol.X[r])


def test_cholesky_rows_alone_inside_the_bound_with_the_batch_bits(chol):
    """Every row as its own call, the long ones included (the partial path alone and in company): inside the bound, and
    the bits it has in the batch."""
    for r in range(chol.pr.N_ROWS):
        X, nf = chol.alone(r)
        assert X.shape == (1, chol.d) and int(nf.item()) == 0
        chol.pr.check_row(r, X[0].cpu().numpy(), tag="alone ")
        assert t.equal(X[0], chol.X_dev[r]), (chol.d, r)


# ---- 2, 3. the block form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,B", WC.ONE_BLOCK_SHAPES)
def test_one_block_inside_the_derived_bound(d, B):
    c = _block(d, B)
    X = c.out(True, 1).cpu().numpy()
    for r, (e, a) in enumerate(zip(c.pr.rows, c.pr.conf)):
        if len(e) == 0:
            assert not X[r].any()
            continue
        reg_r = c.pr.reg_rows[r]
        res, bound = WE.residual(e, a, c.pr.Y, c.pr.G, reg_r, X[r]), WE.residual_bound(e, a, c.pr.Y, c.pr.G, reg_r, X[r])
        print(f"d={d} B={B} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert np.isfinite(X[r]).all() and res <= bound, (d, B, r, res, bound)


@pytest.mark.parametrize("from_zero,sweeps", WC.STARTS)
def test_several_blocks_within_eight_times_the_float32_reference(block, from_zero, sweeps):
    """max_r ||x_kernel - x_64||_2 <= 8 * max_r ||x_f32ref - x_64||_2, the criterion of test_gpu_als_block.py; the measured
    ratios are recorded in profiles/als_weighted.md."""
    X64, _, tol = block.pr.refs(from_zero, sweeps)
    X = block.out(from_zero, sweeps).cpu().numpy().astype(np.float64)
    assert np.isfinite(X).all() and not X[0].any()
    err = np.linalg.norm(X - X64, axis=1)
    print(f"RATIO d={block.d} B={block.B} from_zero={from_zero} sweeps={sweeps}: kernel {err.max():.3e} f32ref {tol / 8:.3e} "
          f"ratio {err.max() / (tol / 8):.2f} (long row {err[block.pr.LONG_ROW]:.3e})")
    assert tol > 0 and err.max() <= tol and err[block.pr.LONG_ROW] <= tol


# ---- 4. constant weights: the unweighted rule -----------------------------------------------------------------------------------
def test_constant_weights_meet_the_unweighted_bound_cholesky(chol):
    pr = chol.pr
    conf = t.full_like(chol.conf_dev, WC.ALPHA)
    reg_rows = t.full_like(chol.reg_dev, WC.REG)
    X, nf = ops.als_solve_rows(chol.csr, chol.Y_dev, chol.G_dev, alpha=9.0, reg=9.0, conf=conf, reg_rows=reg_rows)
    X2, _ = ops.als_solve_rows(chol.csr, chol.Y_dev, chol.G_dev, alpha=WC.ALPHA, reg=WC.REG, reg_rows=reg_rows)   # conf filled
    X3, _ = ops.als_solve_rows(chol.csr, chol.Y_dev, chol.G_dev, alpha=9.0, reg=WC.REG, conf=conf)                # scalar reg
    assert int(nf.item()) == 0 and t.equal(X, X2) and t.equal(X, X3)
    X = X.cpu().numpy()
    for r, e in enumerate(pr.rows):
        if len(e) == 0:
            assert not X[r].any()
            continue
        res, bound = AE.residual(e, pr.Y, pr.G, WC.ALPHA, WC.REG, X[r]), AE.residual_bound(e, pr.Y, pr.G, WC.ALPHA, WC.REG, X[r])
        print(f"constant d={chol.d} row {r} n={len(e)}: residual {res:.3e} unweighted bound {bound:.3e}")
        assert res <= bound, (chol.d, r, res, bound)


@pytest.mark.parametrize("d,B", WC.ONE_BLOCK_SHAPES)
def test_constant_weights_meet_the_unweighted_bound_block(d, B):
    c = _block(d, B)
    pr = c.pr
    X, nf = ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, alpha=9.0, reg=9.0, block=B, conf=t.full_like(c.conf_dev, WC.ALPHA),
                               reg_rows=t.full_like(c.reg_dev, WC.REG))
    assert int(nf.item()) == 0
    X = X.cpu().numpy()
    for r, e in enumerate(pr.rows):
        if len(e):
            res, bound = AE.residual(e, pr.Y, pr.G, WC.ALPHA, WC.REG, X[r]), AE.residual_bound(e, pr.Y, pr.G, WC.ALPHA, WC.REG, X[r])
            assert res <= bound, (d, B, r, res, bound)


def test_constant_weights_block_follows_the_unweighted_float64_sweeps(block):
    """Several blocks: against the UNWEIGHTED float64 mirror within 8 times the unweighted float32 reference's distance."""
    base = WC.BC.problem(block.d, block.B)
    csr, _ = _csr(base.rows, [np.zeros(len(e), dtype=F) for e in base.rows])
    conf = t.full((csr.nnz,), WC.ALPHA, device="cuda")
    X64, _, tol = base.refs(False, 3)
    X, nf = ops.als_block_rows(csr, block.Y_dev, block.G_dev, alpha=9.0, reg=WC.REG, block=block.B, sweeps=3,
                               x=block.X0_dev.clone(), conf=conf)
    err = np.linalg.norm(X.cpu().numpy().astype(np.float64) - X64, axis=1)
    assert int(nf.item()) == 0 and err.max() <= tol


# ---- 5. the exact cases ---------------------------------------------------------------------------------------------------------
def test_exact_cholesky_case():
    Y, G, rows, conf, reg_rows = WC.exact_chol_case()
    csr, cf = _csr(rows, conf, Y.shape[0])
    want = np.stack([WE.x64(e, a, Y, G, reg_rows[r]) for r, (e, a) in enumerate(zip(rows, conf))])
    X, nf = ops.als_solve_rows(csr, _dev(Y), _dev(G), alpha=1.0, reg=1.0, conf=cf, reg_rows=_dev(reg_rows))
    assert int(nf.item()) == 0 and want.any()
    assert t.equal(X.cpu(), t.from_numpy(want.astype(F)))
    assert np.array_equal(want.astype(F).astype(np.float64), want)


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_block_case(sweeps, warm):
    Y, G, rows, conf, reg_rows, X0 = WC.exact_block_case()
    csr, cf = _csr(rows, conf, Y.shape[0])
    want = np.stack([WE.block_sweep64(e, a, Y, G, reg_rows[r], X0[r] if warm else None, 16, sweeps)
                     for r, (e, a) in enumerate(zip(rows, conf))])
    X, nf = ops.als_block_rows(csr, _dev(Y), _dev(G), alpha=1.0, reg=1.0, block=16, sweeps=sweeps, x=_dev(X0) if warm else None,
                               conf=cf, reg_rows=_dev(reg_rows))
    assert int(nf.item()) == 0 and want.any()
    assert t.equal(X.cpu(), t.from_numpy(want.astype(F)))
    assert np.array_equal(want.astype(F).astype(np.float64), want)


# ---- 6. equal bits --------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits(chol):
    X, _ = chol.call()
    assert t.equal(X, chol.X_dev)


def test_two_block_calls_give_equal_bits(block):
    for from_zero, sweeps in WC.STARTS:
        X, _ = block.call(from_zero, sweeps)
        assert t.equal(X, block.out(from_zero, sweeps))


def test_a_block_row_alone_equals_its_bits_in_the_batch(block):
    want = block.out(False, 3)
    for r in range(block.pr.N_ROWS):
        X, _ = block.alone(r, False, 3)
        assert t.equal(X[0], want[r]), (block.d, block.B, r)


def test_row_list_in_any_order_with_reg_rows_by_row_id(chol):
    order = [6, 3, 19, 0, 8, 5, 9, 1]          # the long row, 33, a short one, the empty one, the repeat, L + 1, the zeros, 1
    rl = _dev(np.asarray(order, dtype=np.int32))
    out = t.full((len(order), chol.d), float("nan"), device="cuda")
    X, nf = chol.call(row_list=rl, out=out)
    assert X is out and int(nf.item()) == 0
    assert t.equal(X, chol.X_dev[rl.long()])


def test_block_row_list_in_any_order_with_reg_rows_by_row_id(block):
    order = [block.pr.LONG_ROW, 3, 39, 0, 6, 5, 1, 4, WC.REPEAT_ROW, WC.ZERO_ROW]
    rl = _dev(np.asarray(order, dtype=np.int32))
    for from_zero, sweeps in WC.STARTS:
        X, nf = block.call(from_zero, sweeps, rows=order, row_list=rl)
        assert int(nf.item()) == 0 and X.shape == (len(order), block.d)
        assert t.equal(X, block.out(from_zero, sweeps)[rl.long()])


@pytest.mark.parametrize("d", [16, 128])
def test_direct_and_partial_path_give_the_same_bits(d):
    """A row of L + 3 entries whose last three are a zero factor row (with weights of their own): its chunk 1 is exactly zero,
    so the rule gives it the bits of the L-entry row (S_0 + 0 == S_0, s_0 + 0 == s_0), which takes the direct path."""
    L = ops.als_chunk(d)
    rng = np.random.default_rng(3)
    Y = (rng.standard_normal((50, d)) * 0.3).astype(F)
    Y[49] = 0.0
    G = np.eye(d, dtype=F)
    head = rng.integers(0, 49, L).tolist()
    a = np.exp(rng.uniform(np.log(0.1), np.log(30.0), L)).astype(F)
    csr, cf = _csr([head, head + [49, 49, 49]], [a, np.concatenate([a, F([2.0, 0.5, 7.0])])], 50)
    X, nf = ops.als_solve_rows(csr, _dev(Y), _dev(G), alpha=1.0, reg=1.0, conf=cf, reg_rows=_dev(F([0.75, 0.75])))
    assert int(nf.item()) == 0 and X[0].abs().sum() > 0 and t.equal(X[0], X[1])


@pytest.mark.parametrize("d,B", [(64, 16), (16, 16), (128, 32)])
def test_resident_and_streaming_path_give_the_same_bits(d, B):
    """A row one entry longer than the longest resident row whose last entry is a zero factor row: every chain gains
    fmaf(0, ., acc) == acc, so the rule gives it the bits of the row without that entry.  At d = 16 the weighted kernel's
    own residency limit (128 entries) is below ops.als_block_chunk: both lengths are tried."""
    rng = np.random.default_rng(3)
    Y = (0.2 + rng.standard_normal((50, d)) * 0.3).astype(F)
    Y[49] = 0.0
    G = BE.sym_lower((Y.T @ Y).astype(F))
    for n in sorted({ops.als_block_chunk(d, B), min(ops.als_block_chunk(d, B), 128)}):
        head = rng.integers(0, 49, n).tolist()
        a = np.exp(rng.uniform(np.log(0.1), np.log(30.0), n)).astype(F)
        csr, cf = _csr([head, head + [49]], [a, np.concatenate([a, F([3.0])])], 50)
        x0 = _dev((rng.standard_normal((1, d)) * 0.1).astype(F)).repeat(2, 1)
        X, nf = ops.als_block_rows(csr, _dev(Y), _dev(G), alpha=1.0, reg=1.0, block=B, sweeps=2, x=x0, conf=cf,
                                   reg_rows=_dev(F([1.25, 1.25])))
        assert int(nf.item()) == 0 and X[0].abs().sum() > 0 and t.equal(X[0], X[1]), (d, B, n)


# ---- 7, 8. the unweighted surface is untouched ----------------------------------------------------------------------------------
def test_unweighted_ops_equal_a_direct_call_of_the_old_entries():
    c = _chol(64)
    L = _lib.lib()
    n, d = c.csr.n_rows, 64
    X, nf = ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev, alpha=WC.ALPHA, reg=WC.REG, conf=None, reg_rows=None)
    raw, nfr = t.empty(n, d, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    ws = t.empty(L.mi_als_solve_rows_workspace_bytes(n, c.csr.nnz, d), dtype=t.uint8, device="cuda")
    assert L.mi_als_solve_rows_f32(n, d, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), c.csr.nnz, N_COLS, c.Y_dev.data_ptr(),
                                   d + 8, c.G_dev.data_ptr(), WC.ALPHA, WC.REG, raw.data_ptr(), d, None, 0, nfr.data_ptr(),
                                   ws.data_ptr(), ws.numel(), ops._stream()) == 0
    assert int(nf.item()) == int(nfr.item()) == 0 and t.equal(X, raw)
    b = _block(128, 32)
    n, d = b.csr.n_rows, 128
    Xb, nf = ops.als_block_rows(b.csr, b.Y_dev, b.G_dev, alpha=WC.ALPHA, reg=WC.REG, block=32, sweeps=2, x=b.X0_dev.clone(),
                                conf=None, reg_rows=None)
    raw = b.X0_dev.clone()
    ws = t.empty(L.mi_als_block_rows_workspace_bytes(n, b.csr.nnz, d, 32), dtype=t.uint8, device="cuda")
    assert L.mi_als_block_rows_f32(n, d, 32, 2, b.csr.rowptr.data_ptr(), b.csr.col.data_ptr(), b.csr.nnz, N_COLS,
                                   b.Y_dev.data_ptr(), d + 8, b.G_dev.data_ptr(), WC.ALPHA, WC.REG, raw.data_ptr(), d, 0, None, 0,
                                   nfr.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()) == 0
    assert int(nf.item()) == int(nfr.item()) == 0 and t.equal(Xb, raw)


def _small_graph():
    rng = np.random.default_rng(11)
    pairs = rng.choice(60 * 40, size=400, replace=False)
    return t.from_numpy(np.stack([pairs // 40, pairs % 40]).astype(np.int64))


@pytest.mark.parametrize("solver", ["cholesky", "block"])
def test_model_defaults_give_the_tables_of_a_model_without_the_keywords(solver, monkeypatch):
    """reg_power = 0 and confidence = None: two epochs end in the bits of a model built and fitted without the new keywords,
    and no weighted entry is called on the way."""
    ei = _small_graph().cuda()
    kw = dict(dim=16, alpha=1.0, reg=2.0, seed=5, solver=solver)
    a = ImplicitALS(60, 40, **kw).cuda().fit(Interactions(ei, 60, 40), 2)
    called = []
    L = _lib.lib()
    for name in ("mi_als_solve_rows_w_f32", "mi_als_block_rows_w_f32"):
        monkeypatch.setattr(L, name, lambda *args, _n=name: called.append(_n) or 0)
    b = ImplicitALS(60, 40, reg_power=0.0, **kw).cuda().fit(Interactions(ei, 60, 40), 2, confidence=None)
    assert not called and b._weights is None
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    assert a.objective(Interactions(ei, 60, 40)) == b.objective(Interactions(ei, 60, 40))


# ---- 9. failed rows -------------------------------------------------------------------------------------------------------------
def test_bad_reg_rows_and_broken_pivots_fail_their_row_alone(chol):
    """reg_rows of 0 and NaN on two rows, and on a third a negative conf large enough to break a pivot: three zero rows,
    counted; every other row keeps its bits."""
    reg = chol.reg_dev.clone()
    reg[3], reg[5], reg[0] = 0.0, float("nan"), float("nan")            # row 0 is empty: zero, not counted
    conf = chol.conf_dev.clone()
    lo = int(chol.csr.rowptr[2].item())
    conf[lo:lo + 3] = -1.0e4                                             # row 2 (three entries): A loses its definiteness
    X, nf = ops.als_solve_rows(chol.csr, chol.Y_dev, chol.G_dev, alpha=1.0, reg=1.0, conf=conf, reg_rows=reg)
    assert int(nf.item()) == 3
    keep = [r for r in range(chol.pr.N_ROWS) if r not in (2, 3, 5)]
    assert not X[[2, 3, 5]].cpu().numpy().any() and t.equal(X[keep], chol.X_dev[keep])


def test_bad_reg_rows_and_broken_pivots_fail_their_block_row_alone(block):
    reg = block.reg_dev.clone()
    reg[3], reg[block.pr.LONG_ROW], reg[0] = 0.0, float("nan"), float("inf")
    conf = block.conf_dev.clone()
    lo = int(block.csr.rowptr[2].item())
    conf[lo:lo + 3] = -1.0e4
    X, nf = ops.als_block_rows(block.csr, block.Y_dev, block.G_dev, alpha=1.0, reg=1.0, block=block.B, sweeps=3,
                               x=block.X0_dev.clone(), conf=conf, reg_rows=reg)
    bad = [2, 3, block.pr.LONG_ROW]
    assert int(nf.item()) == 3
    keep = [r for r in range(block.pr.N_ROWS) if r not in bad]
    assert not X[bad].cpu().numpy().any() and t.equal(X[keep], block.out(False, 3)[keep])


def test_c_entries_refuse_on_device_pointers_before_anything_is_enqueued():
    c = _chol(16)
    L = _lib.lib()
    n = c.csr.n_rows
    nf = t.zeros(1, dtype=t.int32, device="cuda")
    X = t.full((n, 16), 7.0, device="cuda")
    ws = t.empty(max(L.mi_als_solve_rows_w_workspace_bytes(n, c.csr.nnz, 16), L.mi_als_block_rows_w_workspace_bytes(n, c.csr.nnz, 16, 16)),
                 dtype=t.uint8, device="cuda")

    def chol(conf=c.conf_dev.data_ptr(), reg_rows=None, reg=1.0):
        return L.mi_als_solve_rows_w_f32(n, 16, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), c.csr.nnz, N_COLS,
                                         c.Y_dev.data_ptr(), 24, c.G_dev.data_ptr(), conf, reg_rows, reg, X.data_ptr(), 16, None, 0,
                                         nf.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())

    def blk(conf=c.conf_dev.data_ptr(), reg_rows=None, reg=1.0):
        return L.mi_als_block_rows_w_f32(n, 16, 16, 1, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), c.csr.nnz, N_COLS,
                                         c.Y_dev.data_ptr(), 24, c.G_dev.data_ptr(), conf, reg_rows, reg, X.data_ptr(), 16, 1, None,
                                         0, nf.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    bad = _lib.MI_ERR_BAD_ARG
    for call in (chol, blk):
        assert call(conf=None) == bad and call(reg=0.0) == bad and call(reg=float("nan")) == bad
    t.cuda.synchronize()
    assert int(nf.item()) == 0 and bool((X == 7.0).all())


# ---- 10. the trainer ------------------------------------------------------------------------------------------------------------
def _weighted_model(solver, ei, w, **kw):
    inter = Interactions(ei.cuda(), 60, 40)
    model = ImplicitALS(60, 40, dim=16, alpha=1.5, reg=0.05, seed=3, reg_power=0.5, solver=solver, **kw).cuda()
    model.bind(inter, w)
    return model, inter


def _sides(ei, w, alpha):
    """Per side: (ptr, idx, a_e by entry position) with a row's entries in edge order, gathered by hand."""
    a = (w.double().numpy() * alpha).astype(F)
    out = []
    for mine, other, n in ((0, 1, 60), (1, 0, 40)):
        rows, cols = ei[mine].numpy(), ei[other].numpy()
        order = np.argsort(rows, kind="stable")
        ptr, idx = AE.csr_of(rows, cols, n)
        out.append((ptr, idx, a[order]))
    return out


def _row_in_device_order(csr, conf_dev, r, ptr, idx, a):
    """The entries of row r in the order of the device CSR, with the weights the DEVICE carries; asserts that they are the
    hand-gathered (column, weight) pairs of that row."""
    lo, hi = int(csr.rowptr[r]), int(csr.rowptr[r + 1])
    cols, cf = csr.col[lo:hi].cpu().numpy(), conf_dev[lo:hi].cpu().numpy()
    hand = sorted(zip(idx[ptr[r]:ptr[r + 1]].tolist(), a[ptr[r]:ptr[r + 1]].tolist()))
    assert sorted(zip(cols.tolist(), cf.tolist())) == hand, r
    return cols.tolist(), cf


def test_trainer_with_confidences_and_reg_power():
    ei = _small_graph()
    rng = np.random.default_rng(5)
    w = t.from_numpy(rng.integers(1, 6, ei.shape[1]).astype(np.float64) * rng.uniform(0.2, 1.0, ei.shape[1]))
    model, inter = _weighted_model("cholesky", ei, w.cuda())
    (ptr_u, idx_u, a_u), (ptr_i, idx_i, a_i) = _sides(ei, w, 1.5)
    a_edge, (conf_u, reg_u), (conf_i, reg_i) = model._weights
    # the regularisers are the formula's, per side
    np.testing.assert_allclose(reg_u.cpu().numpy(), WE.reg_rows64(ptr_u, a_u, 40, 0.05, 0.5), rtol=1e-6)
    np.testing.assert_allclose(reg_i.cpu().numpy(), WE.reg_rows64(ptr_i, a_i, 60, 0.05, 0.5), rtol=1e-6)
    reg_min = float(min(reg_u.min(), reg_i.min()))
    # the device objective is the emulation's
    prev = model.objective(inter)
    want = WE.objective(ptr_u, idx_u, a_u, model.users_emb.weight.cpu().numpy(), model.items_emb.weight.cpu().numpy(),
                        reg_u.cpu().numpy(), reg_i.cpu().numpy())
    assert abs(prev - want) <= 1e-9 * abs(want)
    assert abs(model.objective(Interactions(ei.cuda(), 60, 40), confidence=w.cuda()) - want) <= 1e-9 * abs(want)
    by_user, by_item = model._bound[1], model._bound[2]
    for epoch in range(3):
        for side in ("users", "items"):
            fixed_dev = (model.items_emb if side == "users" else model.users_emb).weight.data.clone()
            assert int(model.half_sweep(side).item()) == 0
            mine = (model.users_emb if side == "users" else model.items_emb).weight.data.cpu().numpy()
            csr, conf_dev, reg_dev, (ptr, idx, a) = ((by_user, conf_u, reg_u, (ptr_u, idx_u, a_u)) if side == "users"
                                                     else (by_item, conf_i, reg_i, (ptr_i, idx_i, a_i)))
            fixed = fixed_dev.cpu().numpy()
            G = ops.gemm(fixed_dev, fixed_dev, trans_a=True, trans_b=False).cpu().numpy()
            G = np.tril(G) + np.tril(G, -1).T
            absf = np.abs(fixed).astype(np.float64)
            extra = AE.g(fixed.shape[0]) * np.linalg.norm(absf.T @ absf, "fro")   # the f32 Gram against the objective's float64 one
            slack = 0.0
            for r in range(csr.n_rows):
                if ptr[r + 1] > ptr[r]:
                    cols, cf = _row_in_device_order(csr, conf_dev, r, ptr, idx, a)   # the right weight on every entry, both sides
                    reg_r = float(reg_dev[r])
                    b = WE.residual_bound(cols, cf, fixed, G, reg_r, mine[r]) + extra * np.linalg.norm(mine[r].astype(np.float64))
                    assert WE.residual(cols, cf, fixed, G, reg_r, mine[r]) <= b, (side, r)   # the row's half-sweep solution
                    slack += b * b
            slack /= 2.0 * reg_min
            cur = model.objective(inter)
            print(f"epoch {epoch} {side}: objective {cur:.9g} (previous {prev:.9g}, slack {slack:.3e})")
            assert cur <= prev + slack
            prev = cur
            if side == "users":   # fold-in of a training row with its weights: that row's half-sweep solution
                for u in (0, 17, 59):
                    lo, hi = int(by_user.rowptr[u]), int(by_user.rowptr[u + 1])
                    p = t.tensor([0, hi - lo], dtype=t.int32, device="cuda")
                    wts = conf_u[lo:hi].double() / 1.5                        # back to w_e: a_e = alpha w_e
                    x = model.fold_in(p, by_user.col[lo:hi].contiguous(), confidence=wts)[0]
                    cols, cf = by_user.col[lo:hi].cpu().tolist(), (wts.cpu().numpy() * 1.5).astype(F)
                    reg_r = float(WE.reg_rows64([0, hi - lo], cf, 40, 0.05, 0.5)[0].astype(F))
                    xr = x.cpu().numpy()
                    assert xr.any() and WE.residual(cols, cf, fixed, G, reg_r, xr) <= WE.residual_bound(cols, cf, fixed, G, reg_r, xr)
    # one item row against the mirror, its weights gathered by hand from the edge list
    i = int(np.argmax(np.diff(ptr_i)))
    users = ei[0][ei[1] == i].numpy()
    wt = (w[ei[1] == i].numpy() * 1.5).astype(F)
    Xd = model.users_emb.weight.data
    G = ops.gemm(Xd, Xd, trans_a=True, trans_b=False).cpu().numpy()
    G = np.tril(G) + np.tril(G, -1).T
    reg_r = float(reg_i[i])                                             # the formula's, asserted above
    assert abs(reg_r - 0.05 * (60 + wt.astype(np.float64).sum()) ** 0.5) <= 1e-6 * reg_r
    before = model.items_emb.weight.data.clone()
    assert int(model.half_sweep("items").item()) == 0
    yi = model.items_emb.weight.data[i].cpu().numpy()
    res = WE.residual(users.tolist(), wt, Xd.cpu().numpy(), G, reg_r, yi)
    bound = WE.residual_bound(users.tolist(), wt, Xd.cpu().numpy(), G, reg_r, yi)
    # the same row with its weights in reversed order is a different system: the bound can tell
    wrong = WE.residual(users.tolist(), wt[::-1].copy(), Xd.cpu().numpy(), G, reg_r, yi)
    print(f"item {i} ({len(users)} entries): residual {res:.3e} bound {bound:.3e}; with the weights reversed {wrong:.3e}")
    assert res <= bound < wrong
    assert t.equal(before, model.items_emb.weight.data)                 # the same user table: the same item half-sweep, bit for bit


def test_block_trainer_with_confidences_runs_the_weighted_entry():
    """solver="block" with weights: every half-sweep lowers the weighted objective (an exact block step never raises a row's
    share; float32 noise is far below the first epochs' decrease), and two fits give equal bits."""
    ei = _small_graph()
    rng = np.random.default_rng(6)
    w = t.from_numpy(rng.uniform(0.0, 4.0, ei.shape[1])).cuda()
    model, inter = _weighted_model("block", ei, w, block=16, block_sweeps=2)
    prev = model.objective(inter)
    for _ in range(2):
        for side in ("users", "items"):
            assert int(model.half_sweep(side).item()) == 0
            cur = model.objective(inter)
            assert cur < prev
            prev = cur
    a = ImplicitALS(60, 40, dim=16, alpha=1.5, reg=0.05, seed=3, reg_power=0.5, solver="block").cuda().fit(inter, 2, confidence=w)
    b = ImplicitALS(60, 40, dim=16, alpha=1.5, reg=0.05, seed=3, reg_power=0.5, solver="block").cuda().fit(inter, 2, confidence=w)
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    c = ImplicitALS(60, 40, dim=16, alpha=1.5, reg=0.05, seed=3, reg_power=0.5, solver="block").cuda().fit(inter, 2)
    assert not t.equal(a.users_emb.weight, c.users_emb.weight)          # the weights do reach the solver
