"""GPU: the hub path of the iALS block row solver (mi_als_block_rows_hub_f32 and its weighted twin, csrc/als_block.hip) against
the float64 statement of the block rule: hub rows within 8 times the committed float32 block reference's distance, inside the
derived bound where one block is the whole row, an exact case, determinism and row purity, the chunk boundary, the bits of
the rows that are no hub rows, failed rows (a NaN, a bad regulariser, hub counts too small), refusals, and
als.ImplicitALS(solver="block", hub_threshold=) end to end.  Every test here needs the keyword."""
import numpy as np
import pytest
import torch as t

import als_block_cases as BC
import als_block_emulation as BE
import als_emulation as AE
import als_hub_cases as HC
import als_hub_emulation as HE
import als_weighted_emulation as WE
from laplace_amd import _lib, ops, synthetic as S
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions
from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn

pytestmark = pytest.mark.gpu

ALPHA, REG = HC.ALPHA, HC.REG
N_TABLE = HC.N_COLS + 1                       # the problems' table: N_COLS rows and the zero row


def _dev(a, dtype=None):
    x = t.from_numpy(np.ascontiguousarray(a)).cuda()
    return x if dtype is None else x.to(dtype)


def _csr(rows, n_cols):
    ptr, idx = HC.csr_arrays(rows)
    return ops.DeviceCSR(len(rows), n_cols, _dev(ptr), _dev(idx))


class Case:
    """The device side of one HC.Problem (or WeightedProblem): the operands and one batched call per (start, threshold)."""

    def __init__(self, pr, weighted=False):
        self.pr, self.d, self.B, self.weighted = pr, pr.d, pr.B, weighted
        self.Y_dev = _dev(pr.wide)[:, 4:4 + pr.d]
        self.G_dev = _dev(pr.G)
        self.X0_dev = _dev(pr.X0)
        self.csr = _csr(pr.rows, N_TABLE)
        if weighted:
            self.conf_dev = _dev(np.concatenate(pr.conf))
            self.reg_dev = _dev(pr.reg_rows)
        self._out = {}

    def call(self, from_zero, sweeps, thr, csr=None, rows=None, row_list=None, with_reg_rows=True):
        x = None
        if not from_zero:
            x = self.X0_dev.clone() if rows is None else self.X0_dev[rows].clone()
        kw = {}
        if self.weighted:
            assert csr is None
            kw = dict(conf=self.conf_dev, reg_rows=self.reg_dev if with_reg_rows else None)
        return ops.als_block_rows(csr or self.csr, self.Y_dev, self.G_dev, alpha=ALPHA, reg=REG, block=self.B, sweeps=sweeps,
                                  x=x, row_list=row_list, hub_threshold=thr, **kw)

    def out(self, from_zero, sweeps, thr, with_reg_rows=True):
        """thr None: the plain block entry."""
        key = (from_zero, sweeps, thr, with_reg_rows)
        if key not in self._out:
            X, nf = self.call(from_zero, sweeps, thr, with_reg_rows=with_reg_rows)
            assert int(nf.item()) == 0
            self._out[key] = X
        return self._out[key]


_CASES = {}


def _case(d, B, weighted=False):
    key = (d, B, weighted)
    if key not in _CASES:
        _CASES[key] = Case(HC.weighted_problem(d, B) if weighted else HC.problem(d, B), weighted)
    return _CASES[key]


@pytest.fixture(params=HC.SHAPES, ids=lambda s: f"d{s[0]}-B{s[1]}")
def case(request):
    return _case(*request.param)


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------
def _check_accuracy(tag, pr, X, X64, err32, thr):
    X = X.cpu().numpy().astype(np.float64)
    assert np.isfinite(X).all() and not X[0].any()
    err = np.linalg.norm(X - X64, axis=1)
    groups = [("all", list(range(pr.n_rows))), ("hub", pr.hub_rows(thr))] + ([("multi-chunk", pr.multi)] if pr.multi else [])
    for name, rows in groups:
        ref = err32[rows].max()
        print(f"RATIO {tag} T={thr} {name} rows: kernel {err[rows].max():.3e} f32ref {ref:.3e} ratio {err[rows].max() / ref:.2f}")
    for name, rows in groups:
        assert err32[rows].max() > 0 and err[rows].max() <= 8.0 * err32[rows].max(), (tag, thr, name)


@pytest.mark.parametrize("thr", HC.THRESHOLDS)
@pytest.mark.parametrize("from_zero,sweeps", BC.STARTS)
def test_within_eight_times_the_float32_reference(case, from_zero, sweeps, thr):
    """max_r ||x_kernel - x_64||_2 <= 8 * max_r ||x_f32ref - x_64||_2 with x_f32ref the committed block_sweep_f32: over all rows of
    the call, over the hub rows, and over the rows of several chunks on their own."""
    assert case.Y_dev.stride(0) == case.d + 8
    X64, err32 = case.pr.refs(from_zero, sweeps)
    _check_accuracy(f"d={case.d} B={case.B} from_zero={from_zero} sweeps={sweeps}", case.pr, case.out(from_zero, sweeps, thr),
                    X64, err32, thr)


@pytest.mark.parametrize("with_reg_rows", [True, False])
@pytest.mark.parametrize("from_zero,sweeps", BC.STARTS)
@pytest.mark.parametrize("d,B", HC.W_SHAPES)
def test_weighted_within_eight_times_the_float32_reference(d, B, from_zero, sweeps, with_reg_rows):
    c = _case(d, B, True)
    X64, err32 = c.pr.refs_w(from_zero, sweeps, with_reg_rows)
    for thr in HC.THRESHOLDS:
        _check_accuracy(f"weighted d={d} B={B} from_zero={from_zero} sweeps={sweeps} reg_rows={with_reg_rows}", c.pr,
                        c.out(from_zero, sweeps, thr, with_reg_rows), X64, err32, thr)


@pytest.mark.parametrize("d,B", [(16, 16), (64, 64)])
def test_one_block_inside_the_derived_bound(d, B):
    """d <= B, a zero start, one sweep: the one block step solves A x = b of the Cholesky entries, whose formation this is
    (the roundings are counted in tests/als_hub_emulation.py)."""
    c = _case(d, B)
    X = c.out(True, 1, 4).cpu().numpy()
    for r in c.pr.hub_rows(4):
        e = c.pr.rows[r]
        res, bound = AE.residual(e, c.pr.Y, c.pr.G, ALPHA, REG, X[r]), AE.residual_bound(e, c.pr.Y, c.pr.G, ALPHA, REG, X[r])
        print(f"d={d} B={B} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert np.isfinite(X[r]).all() and res <= bound, (d, B, r, res, bound)
    w = _case(d, B, True)
    X = w.out(True, 1, 4).cpu().numpy()
    for r in w.pr.hub_rows(4):
        e, a, reg_r = w.pr.rows[r], w.pr.conf[r], w.pr.reg_rows[r]
        res, bound = WE.residual(e, a, w.pr.Y, w.pr.G, reg_r, X[r]), WE.residual_bound(e, a, w.pr.Y, w.pr.G, reg_r, X[r])
        print(f"weighted d={d} B={B} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert np.isfinite(X[r]).all() and res <= bound, (d, B, r, res, bound)


# ---- 2. the exact case ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_case(sweeps, warm):
    """als_block_cases.exact_case, every row of more than 2 entries a hub row: every float32 operation of the hub rule is exact
    there (tests/test_als_hub_cpu.py), so the kernel equals the float64 mirror."""
    Y, G, rows, X0 = BC.exact_case()
    want = np.stack([HE.hub_sweep64(e, Y, G, 1.0, 1.0, X0[r] if warm else None, 16, sweeps) for r, e in enumerate(rows)])
    X, nf = ops.als_block_rows(_csr(rows, Y.shape[0]), _dev(Y), _dev(G), alpha=1.0, reg=1.0, block=16, sweeps=sweeps,
                               x=_dev(X0) if warm else None, hub_threshold=2)
    assert int(nf.item()) == 0 and want.any() and sum(len(e) > 2 for e in rows) >= 8
    assert t.equal(X.cpu(), t.from_numpy(want.astype(np.float32)))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


# ---- 3. determinism, row purity, the threshold, the chunk boundary -------------------------------------------------------------
def test_two_calls_give_equal_bits(case):
    for from_zero, sweeps in ((True, 1), (False, 3)):
        X, _ = case.call(from_zero, sweeps, 4)
        assert t.equal(X, case.out(from_zero, sweeps, 4))


def test_a_hub_row_alone_and_at_another_threshold(case):
    """Every hub row as its own one-row CSR with the threshold n - 1 (still a hub row): the bits it has in the batch at
    threshold 4; and both thresholds of the batch agree on the rows that are hub rows under both."""
    want = case.out(False, 3, 4)
    for r in case.pr.hub_rows(4):
        e = case.pr.rows[r]
        X, nf = case.call(False, 3, len(e) - 1, csr=_csr([e], N_TABLE), rows=[r])
        assert int(nf.item()) == 0 and t.equal(X[0], want[r]), (case.d, case.B, r)
    both = case.pr.hub_rows(64)
    assert len(both) >= 2 and t.equal(case.out(False, 3, 64)[both], want[both])


def test_row_list_in_any_order(case):
    pr = case.pr
    picks = [pr.named[65], 7, 3, 0, pr.named[5], 6, pr.named[4], 1, pr.named[64], 5] + pr.multi[::-1]
    rl = _dev(np.asarray(picks, dtype=np.int32))
    for from_zero, sweeps in ((True, 1), (False, 3)):
        X, nf = case.call(from_zero, sweeps, 4, rows=picks, row_list=rl)
        assert int(nf.item()) == 0 and X.shape == (len(picks), case.d)
        assert t.equal(X, case.out(from_zero, sweeps, 4)[rl.long()])        # compact by list position, the batched call's bits


@pytest.mark.parametrize("d,B", HC.MULTI_CHUNK)
def test_chunk_boundary(d, B):
    """A row of L_h + 1 entries whose last entry is a zero factor row has the bits of the L_h-entry row: every chain gains
    fmaf(0, ., acc) == acc, and the second chunk adds zeros."""
    c = _case(d, B)
    one, two = c.pr.boundary
    assert len(c.pr.rows[one]) == c.pr.L and len(c.pr.rows[two]) == c.pr.L + 1 and not c.pr.Y[c.pr.rows[two][-1]].any()
    for from_zero, sweeps in ((True, 1), (False, 3)):
        X = c.out(from_zero, sweeps, 4)
        assert X[one].abs().sum() > 0 and t.equal(X[one], X[two])


def test_other_rows_and_the_default_keep_the_plain_bits(case):
    pr = case.pr
    for from_zero, sweeps in ((True, 1), (False, 3)):
        plain = case.out(from_zero, sweeps, None)
        direct, _ = ops.als_block_rows(case.csr, case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG, block=case.B, sweeps=sweeps,
                                       x=None if from_zero else case.X0_dev.clone())
        assert t.equal(plain, direct)                                        # hub_threshold=None is the call without the keyword
        for thr in HC.THRESHOLDS:
            rest = [r for r in range(pr.n_rows) if len(pr.rows[r]) <= thr]
            assert t.equal(case.out(from_zero, sweeps, thr)[rest], plain[rest])
            assert not t.equal(case.out(from_zero, sweeps, thr), plain)      # the hub rows did take another path
        longest = max(len(e) for e in pr.rows)
        for thr in (longest, longest + 1, 1 << 40):
            X, nf = case.call(from_zero, sweeps, thr)
            assert int(nf.item()) == 0 and t.equal(X, plain)


# ---- 4. failed rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,B", [(16, 16), (256, 16)])
def test_nan_row_and_empty_row(d, B):
    """A NaN factor row inside a hub row: that row is zero and counted once, its neighbours keep their bits, the empty row is
    zero and not counted.  Arithmetic, no fault."""
    c = _case(d, B)
    pr = c.pr
    wide = np.concatenate([pr.wide, np.full((1, d + 8), np.nan, dtype=np.float32)])
    Y = _dev(wide)[:, 4:4 + d]
    picks = [6, pr.multi[2], 0, 5, pr.named[65]]
    rows = [list(pr.rows[r]) for r in picks]
    good, _ = ops.als_block_rows(_csr(rows, N_TABLE + 1), Y, c.G_dev, alpha=ALPHA, reg=REG, block=B, sweeps=2,
                                 x=c.X0_dev[picks].clone(), hub_threshold=4)
    rows[1][len(rows[1]) // 2] = N_TABLE                                      # the multi-chunk row meets the NaN row
    X, nf = ops.als_block_rows(_csr(rows, N_TABLE + 1), Y, c.G_dev, alpha=ALPHA, reg=REG, block=B, sweeps=2,
                               x=c.X0_dev[picks].clone(), hub_threshold=4)
    assert int(nf.item()) == 1 and not X[1].any() and not X[2].any() and good[1].abs().sum() > 0
    assert t.equal(X[[0, 3, 4]], good[[0, 3, 4]])


def test_bad_reg_rows_on_a_hub_row():
    c = _case(40, 16, True)
    reg = c.reg_dev.clone()
    bad = [6, c.pr.named[65], 0]                                              # two hub rows and the empty row
    reg[bad] = t.tensor([0.0, float("nan"), -1.0], device="cuda")
    X, nf = ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, alpha=ALPHA, reg=REG, block=16, sweeps=3, x=c.X0_dev.clone(),
                               conf=c.conf_dev, reg_rows=reg, hub_threshold=4)
    want = c.out(False, 3, 4)
    keep = [r for r in range(c.pr.n_rows) if r not in bad]
    assert int(nf.item()) == 2 and not X[bad].any() and t.equal(X[keep], want[keep])


@pytest.mark.parametrize("d,B", [(16, 16), (256, 16)])
@pytest.mark.parametrize("short", ["rows", "chunks"])
def test_hub_counts_too_small(d, B, short):
    """The C entry with hub counts below the truth: the rows that found no slot are zero and counted, every other row has its
    bits, and nothing behind the workspace's size is written (a fill pattern guards the tail)."""
    c = _case(d, B)
    pr, L = c.pr, _lib.lib()
    want = c.out(False, 3, 4)
    hub = pr.hub_rows(4)
    n_rows_true, n_chunks_true = ops.als_hub_counts(c.csr, 4, d)
    assert n_rows_true == len(hub) and n_chunks_true == sum(-(-len(pr.rows[r]) // pr.L) for r in hub)
    hr, hc = (n_rows_true - 3, n_chunks_true) if short == "rows" else (n_rows_true, n_chunks_true - 4)
    need = L.mi_als_block_rows_hub_workspace_bytes(pr.n_rows, c.csr.nnz, d, B, hr, hc)
    ws = t.full((need + 4096,), 0xA5, dtype=t.uint8, device="cuda")
    X = c.X0_dev.clone()
    nf = t.zeros(1, dtype=t.int32, device="cuda")
    rc = L.mi_als_block_rows_hub_f32(pr.n_rows, d, B, 3, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), c.csr.nnz, N_TABLE,
                                     c.Y_dev.data_ptr(), d + 8, c.G_dev.data_ptr(), ALPHA, REG, X.data_ptr(), d, 0, None, 0, 4,
                                     hr, hc, nf.data_ptr(), ws.data_ptr(), need, ops._stream())
    assert rc == 0
    zero = [r for r in hub if not X[r].any()]
    print(f"d={d} short {short}: {len(zero)} of {len(hub)} hub rows found no slot")
    assert int(nf.item()) == len(zero) and (len(zero) >= 3 if short == "rows" else len(zero) >= 1)
    keep = [r for r in range(pr.n_rows) if r not in zero]
    assert t.equal(X[keep], want[keep])
    assert bool((ws[need:] == 0xA5).all())


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = _case(16, 16)
    kw = dict(alpha=1.0, reg=1.0)
    for bad in (0, -1, True, 2.5, "4"):
        with pytest.raises(ValueError, match="hub_threshold"):
            ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, hub_threshold=bad, **kw)
    with pytest.raises(ValueError, match="hub_threshold"):
        ImplicitALS(6, 5, dim=16, solver="cholesky", hub_threshold=4)
    # the C entries on real device pointers: by return code, before anything is enqueued
    L = _lib.lib()
    n_rows, nnz = c.pr.n_rows, c.csr.nnz
    hr, hc = ops.als_hub_counts(c.csr, 4, 16)
    nf = t.zeros(1, dtype=t.int32, device="cuda")
    X = t.full((n_rows, 16), 7.0, device="cuda")
    ws = t.empty(L.mi_als_block_rows_hub_workspace_bytes(n_rows, nnz, 16, 16, hr, hc), dtype=t.uint8, device="cuda")
    conf = t.ones(nnz, device="cuda")

    def call(w=False, d=16, block=16, sweeps=1, ldy=24, nnz=nnz, alpha=1.0, reg=1.0, thr=4, hr=hr, hc=hc, ws_bytes=ws.numel()):
        head = (n_rows, d, block, sweeps, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), nnz, N_TABLE, c.Y_dev.data_ptr(), ldy,
                c.G_dev.data_ptr())
        tail = (X.data_ptr(), 16, 0, None, 0, thr, hr, hc, nf.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
        if w:
            return L.mi_als_block_rows_hub_w_f32(*head, conf.data_ptr(), None, reg, *tail)
        return L.mi_als_block_rows_hub_f32(*head, alpha, reg, *tail)
    bad = _lib.MI_ERR_BAD_ARG
    for w in (False, True):
        assert call(w, thr=0) == bad and call(w, thr=-5) == bad and call(w, thr=1 << 31) == bad
        assert call(w, hr=-1) == bad and call(w, hc=-1) == bad and call(w, hr=1 << 31) == bad and call(w, hc=1 << 31) == bad
        assert call(w, d=6) == bad and call(w, d=260) == bad and call(w, block=8) == bad and call(w, sweeps=65) == bad
        assert call(w, nnz=1 << 31) == bad and call(w, ldy=18) == bad and call(w, reg=0.0) == bad
        assert call(w, ws_bytes=ws.numel() - 256) == _lib.MI_ERR_WORKSPACE
        assert call(w, hr=hr + 1) == _lib.MI_ERR_WORKSPACE and call(w, hc=hc + 64) == _lib.MI_ERR_WORKSPACE
    assert call(alpha=-1.0) == bad
    t.cuda.synchronize()
    assert int(nf.item()) == 0 and bool((X == 7.0).all())             # nothing was enqueued


# ---- 6. the trainer -------------------------------------------------------------------------------------------------------------
def _small_graph():
    rng = np.random.default_rng(11)
    pairs = rng.choice(60 * 50, size=500, replace=False)
    return t.from_numpy(np.stack([pairs // 50, pairs % 50]).astype(np.int64))


def test_trainer_at_dim_256_follows_the_float64_half_sweeps():
    """test_gpu_als_block.py's criterion with hub_threshold=4 (most rows of the 60 x 50 graph are hub rows then): after each
    half-sweep the device objective agrees with the objective after a float64 block half-sweep from the same start, within 8
    times the relative gap the float32 reference leaves."""
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 50)
    alpha, reg, B = 1.0, 2.0, 16
    model = ImplicitALS(60, 50, dim=256, alpha=alpha, reg=reg, seed=3, solver="block", block=B, hub_threshold=4).cuda()
    ptr_u, idx_u = AE.csr_of(ei[0].numpy(), ei[1].numpy(), 60)
    ptr_i, idx_i = AE.csr_of(ei[1].numpy(), ei[0].numpy(), 50)
    assert (np.diff(ptr_u) > 4).sum() > 40 and (np.diff(ptr_i) > 4).sum() > 40
    for epoch in range(2):
        for side in ("users", "items"):
            X0, Y0 = model.users_emb.weight.cpu().numpy(), model.items_emb.weight.cpu().numpy()
            assert int(model.half_sweep(side, inter).item()) == 0
            got = model.objective(inter)
            (ptr, idx, mine, fixed) = (ptr_u, idx_u, X0, Y0) if side == "users" else (ptr_i, idx_i, Y0, X0)
            f64 = fixed.astype(np.float64)
            new64 = BE.half_sweep(BE.block_sweep64, ptr, idx, fixed, f64.T @ f64, alpha, reg, mine, B, 1)
            new32 = BE.half_sweep(BE.block_sweep_f32, ptr, idx, fixed, fixed.T @ fixed, alpha, reg, mine, B, 1)
            objs = [AE.objective(ptr_u, idx_u, *((new, Y0) if side == "users" else (X0, new)), alpha, reg) for new in (new64, new32)]
            gap_ref, gap = abs(objs[1] - objs[0]) / abs(objs[0]), abs(got - objs[0]) / abs(objs[0])
            print(f"epoch {epoch} {side}: objective {got:.10g}, float64 {objs[0]:.10g}, float32 reference {objs[1]:.10g}: "
                  f"relative gap {gap:.3e} against {gap_ref:.3e}")
            assert gap <= 8 * gap_ref


def test_trainer_fit_fold_in_and_confidence():
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 50)
    kw = dict(dim=256, alpha=1.0, reg=2.0, seed=5, solver="block", hub_threshold=4)
    a = ImplicitALS(60, 50, **kw).cuda().fit(inter, 2)
    b = ImplicitALS(60, 50, **kw).cuda().fit(Interactions(ei.cuda(), 60, 50), 2)
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    assert t.isfinite(a.users_emb.weight).all() and a.users_emb.weight.abs().sum() > 0
    plain = ImplicitALS(60, 50, **dict(kw, hub_threshold=None)).cuda().fit(inter, 2)
    assert not t.equal(a.users_emb.weight, plain.users_emb.weight)           # the keyword does reach the half-sweeps
    # fold_in with and without the keyword, both against the float64 block rule from zero, inside the float32 yardstick
    csr = inter.csr()
    Y = a.items_emb.weight.cpu().numpy()
    G64, G32 = Y.astype(np.float64).T @ Y.astype(np.float64), Y.T @ Y
    for u in (0, 17, 59):
        lo, hi = int(csr.rowptr[u]), int(csr.rowptr[u + 1])
        assert hi - lo > 4
        p, idx = t.tensor([0, hi - lo], dtype=t.int32, device="cuda"), csr.col[lo:hi].contiguous()
        e = idx.cpu().numpy()
        x64 = BE.block_sweep64(e, Y, G64, 1.0, 2.0, None, 16, a.fold_in_sweeps)
        tol = 8.0 * np.linalg.norm(BE.block_sweep_f32(e, Y, G32, 1.0, 2.0, None, 16, a.fold_in_sweeps).astype(np.float64) - x64)
        a.hub_threshold = 4
        with_hub = a.fold_in(p, idx)[0].cpu().numpy().astype(np.float64)
        a.hub_threshold = None
        without = a.fold_in(p, idx)[0].cpu().numpy().astype(np.float64)
        a.hub_threshold = 4
        print(f"user {u}: fold_in with the hub path {np.linalg.norm(with_hub - x64):.3e}, without {np.linalg.norm(without - x64):.3e}"
              f", tolerance {tol:.3e}")
        assert np.linalg.norm(with_hub - x64) <= tol and np.linalg.norm(without - x64) <= tol
    # per-edge confidences and the frequency-scaled regulariser: the weighted hub entry, no failed rows
    w = t.from_numpy(np.random.default_rng(2).uniform(0.5, 3.0, ei.shape[1])).cuda()
    m = ImplicitALS(60, 50, reg_power=0.5, **dict(kw, reg=0.2)).cuda().fit(inter, 2, confidence=w)   # raises on a failed row
    m2 = ImplicitALS(60, 50, reg_power=0.5, **dict(kw, reg=0.2, hub_threshold=None)).cuda().fit(inter, 2, confidence=w)
    assert t.isfinite(m.users_emb.weight).all() and not t.equal(m.users_emb.weight, m2.users_emb.weight)
    rel = float((m.users_emb.weight - m2.users_emb.weight).norm() / m2.users_emb.weight.norm())
    print(f"weighted fit, hub path against plain block solver: relative distance of the user tables {rel:.3e}")


# ---- 7. quality -----------------------------------------------------------------------------------------------------------------
def test_planted_graph_beats_popularity():
    """test_gpu_als_block.py's recipe with hub_threshold=256 (the longest item row of this graph has 785 entries)."""
    spec = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).cuda()
    inter = Interactions(ei.cuda(), spec.num_users, spec.num_items)
    kw = dict(dim=64, alpha=1.0, reg=20.0, seed=0, solver="block")
    model = ImplicitALS(spec.num_users, spec.num_items, hub_threshold=256, **kw).cuda().fit(inter, 5)
    n_hub = sum(ops.als_hub_counts(model._bound[k], 256, 64)[0] for k in (1, 2))
    m_hub = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], ks=(12,))["map@12"]
    plain = ImplicitALS(spec.num_users, spec.num_items, **kw).cuda().fit(inter, 5)
    m_plain = get_full_rank_metrics_lightgcn(plain, held, [inter.edge_index], ks=(12,))["map@12"]
    deg = t.bincount(inter.edge_index[1], minlength=spec.num_items).to(t.float32)
    ue = t.zeros(spec.num_users, 4, device="cuda")
    ue[:, 0] = 1.0
    ie = t.zeros(spec.num_items, 4, device="cuda")
    ie[:, 0] = deg
    m_pop = get_full_rank_metrics_lightgcn(None, held, [inter.edge_index], ks=(12,), embeddings=(ue, ie))["map@12"]
    print(f"map@12: iALS block with hub_threshold=256 ({n_hub} hub rows) {m_hub:.4f}, plain block solver {m_plain:.4f}, "
          f"popularity {m_pop:.4f}")
    assert n_hub > 0 and m_hub > m_pop
