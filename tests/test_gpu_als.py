"""GPU: the implicit-ALS row solves (mi_als_solve_rows_f32, csrc/als.hip) against the float64 statement of their rule inside the
derived bound (tests/als_emulation.py), an exact case, determinism and row purity across the direct and the partial path,
failed pivots, refusals, and als.ImplicitALS end to end: objective, fold-in, the consumers of LightGCN's tables, and MAP@12 on
the planted C1-scale graph against the popularity predictor."""
import numpy as np
import pytest
import torch as t

import als_emulation as AE
from laplace_amd import _lib, ops, synthetic as S
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions
from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn, topk_for_users

pytestmark = pytest.mark.gpu

ALPHA, REG = 1.5, 0.75
N_COLS, N_ROWS = 300, 70
DIMS = (4, 16, 64, 128)
ROW_LIST = [6, 3, 69, 0, 8, 5, 7]   # the long row, L - 1, a short one, the empty one, the repeated entry, L + 1, one item only


def _dev(a, dtype=None):
    x = t.from_numpy(np.ascontiguousarray(a)).cuda()
    return x if dtype is None else x.to(dtype)


def _csr(rows, n_cols):
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ops.DeviceCSR(len(rows), n_cols, _dev(ptr), _dev(idx))


class Case:
    """One width: the edge rows of the rule (lengths 0, 1, 2, L - 1, L, L + 1, 3 L + 5, one item only, a repeated entry) and
    random short ones up to 70 rows, over a column slice (ldy = d + 8) of a wider table; one batched solve and its float64
    references, shared by the tests below."""

    def __init__(self, d):
        rng = np.random.default_rng(100 + d)
        self.d, self.L = d, ops.als_chunk(d)
        L = self.L
        lens = [0, 1, 2, L - 1, L, L + 1, 3 * L + 5]
        rows = [rng.integers(0, N_COLS, n).tolist() for n in lens]
        rows.append([5] * 7)                                   # every entry names one item
        rows.append([11, 42, 7, 42, 3, 250])                   # a repeated entry
        rows += [rng.integers(0, N_COLS, n).tolist() for n in rng.integers(1, 40, N_ROWS - len(rows))]
        self.rows = rows
        wide = (0.25 + rng.standard_normal((N_COLS, d + 8)) * 0.2).astype(np.float32)
        self.Y = wide[:, 4:4 + d]                              # numpy view; the device tensor is the same slice
        self.Y_dev = _dev(wide)[:, 4:4 + d]
        G = self.Y.astype(np.float64).T @ self.Y.astype(np.float64)
        self.G = (0.5 * (G + G.T)).astype(np.float32)
        self.G = np.tril(self.G) + np.tril(self.G, -1).T       # exactly symmetric in float32
        self.G_dev = _dev(self.G)
        self.csr = _csr(rows, N_COLS)
        X, nf = ops.als_solve_rows(self.csr, self.Y_dev, self.G_dev, alpha=ALPHA, reg=REG)
        self.X_dev, self.X, self.n_failed = X, X.cpu().numpy(), int(nf.item())

    def check_row(self, r, x):
        e = self.rows[r]
        if len(e) == 0:
            assert not x.any(), r
            return
        assert np.isfinite(x).all(), r
        res, bound = AE.residual(e, self.Y, self.G, ALPHA, REG, x), AE.residual_bound(e, self.Y, self.G, ALPHA, REG, x)
        print(f"d={self.d} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert res <= bound, (self.d, r, len(e), res, bound)


_CASES = {}


@pytest.fixture(params=DIMS)
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


# ---- 1. against float64, inside the bound ---------------------------------------------------------------------------------------
def test_batched_solve_inside_the_bound(case):
    assert case.Y_dev.stride(0) == case.d + 8 and case.n_failed == 0
    for r in range(N_ROWS):
        case.check_row(r, case.X[r])


def test_single_row_call_inside_the_bound(case):
    """n_rows = 1: the long row alone."""
    X, nf = ops.als_solve_rows(_csr([case.rows[6]], N_COLS), case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG)
    assert X.shape == (1, case.d) and int(nf.item()) == 0
    case.check_row(6, X[0].cpu().numpy())


def test_row_list_in_any_order(case):
    rl = _dev(np.asarray(ROW_LIST, dtype=np.int32))
    out = t.full((len(ROW_LIST), case.d), float("nan"), device="cuda")
    X, nf = ops.als_solve_rows(case.csr, case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG, row_list=rl, out=out)
    assert X is out and int(nf.item()) == 0
    got = X.cpu().numpy()
    for p, r in enumerate(ROW_LIST):
        case.check_row(r, got[p])
    assert t.equal(X, case.X_dev[rl.long()])                  # compact by list position, the batched call's bits


@pytest.mark.parametrize("d", [8, 20, 40, 96, 116])
def test_widths_between_the_classes(d):
    """Widths that are no multiple of 16, or fill their width class only partly: short rows and one long row, inside the bound."""
    rng = np.random.default_rng(d)
    L = ops.als_chunk(d)
    rows = [rng.integers(0, 80, n).tolist() for n in (0, 1, 3, 17, 33, 64, L + 7)]
    Y = (0.25 + rng.standard_normal((80, d)) * 0.2).astype(np.float32)
    G = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    G = np.tril(G) + np.tril(G, -1).T
    X, nf = ops.als_solve_rows(_csr(rows, 80), _dev(Y), _dev(G), alpha=ALPHA, reg=REG)
    X = X.cpu().numpy()
    assert int(nf.item()) == 0 and not X[0].any()
    for r in range(1, len(rows)):
        res, bound = AE.residual(rows[r], Y, G, ALPHA, REG, X[r]), AE.residual_bound(rows[r], Y, G, ALPHA, REG, X[r])
        print(f"d={d} row {r} n={len(rows[r])}: residual {res:.3e} bound {bound:.3e}")
        assert np.isfinite(X[r]).all() and res <= bound, (d, r, res, bound)


# ---- 2. an exact case -----------------------------------------------------------------------------------------------------------
def test_exact_diagonal_case():
    """One-hot item rows with small integer entries, a diagonal G, alpha = 1, reg = 1: A = diag(m_j^2 + G_jj + 1) with G chosen
    so that every entry is a power of FOUR (its square root and the reciprocal of that are exact), b_j = +-2 m_j: every
    operation of the rule and of the factorisation is exact, so x == b / diag(A) bit for bit."""
    d, per_col = 16, 3
    rng = np.random.default_rng(7)
    mag = np.array([1, 2, 3, 5] * 4, dtype=np.float32)                 # |entry| of the items of column j
    diag_a = np.array([4, 16, 16, 64] * 4, dtype=np.float32)
    Y = np.zeros((d * per_col, d), dtype=np.float32)
    sign = rng.choice([-1.0, 1.0], size=d * per_col).astype(np.float32)
    for j in range(d):
        for c in range(per_col):
            Y[j * per_col + c, j] = sign[j * per_col + c] * mag[j]
    G = np.diag(diag_a - mag * mag - 1.0).astype(np.float32)
    rows = []
    for _ in range(20):                                                # one item of every column, in a random order
        pick = [j * per_col + int(rng.integers(per_col)) for j in range(d)]
        rows.append(rng.permutation(pick).tolist())
    X, nf = ops.als_solve_rows(_csr(rows, d * per_col), _dev(Y), _dev(G), alpha=1.0, reg=1.0)
    want = np.stack([2.0 * Y[r].sum(axis=0) / diag_a for r in rows]).astype(np.float32)
    assert int(nf.item()) == 0 and t.equal(X.cpu(), t.from_numpy(want))


# ---- 3. determinism and row purity ----------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits(case):
    X, _ = ops.als_solve_rows(case.csr, case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG)
    assert t.equal(X, case.X_dev)


def test_a_row_alone_equals_its_bits_in_the_batch(case):
    """Every row as its own one-row CSR, the long ones included: the partial path alone and in company."""
    for r in range(N_ROWS):
        X, _ = ops.als_solve_rows(_csr([case.rows[r]], N_COLS), case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG)
        assert t.equal(X[0], case.X_dev[r]), (case.d, r)


def test_direct_and_partial_path_agree_with_the_rule():
    """A row of L + 3 entries whose last three are a zero factor row: its chunk 1 is exactly zero, so the rule gives it the bits
    of the L-entry row (S_0 + 0 == S_0), which takes the direct path."""
    d = 16
    L = ops.als_chunk(d)
    rng = np.random.default_rng(3)
    Y = (rng.standard_normal((50, d)) * 0.3).astype(np.float32)
    Y[49] = 0.0
    G = np.eye(d, dtype=np.float32)
    head = rng.integers(0, 49, L).tolist()
    X, nf = ops.als_solve_rows(_csr([head, head + [49, 49, 49]], 50), _dev(Y), _dev(G), alpha=ALPHA, reg=REG)
    assert int(nf.item()) == 0 and t.equal(X[0], X[1])


# ---- 4. failed pivots -----------------------------------------------------------------------------------------------------------
def test_failed_pivots_are_counted_and_zeroed(case):
    G_bad = _dev(-10.0 * np.eye(case.d, dtype=np.float32))
    rows = [case.rows[r] for r in (0, 1, 2, 7, 8, 5, 20, 0)]          # two empty rows among them, and a long one (L + 1)
    out = t.full((len(rows), case.d), float("nan"), device="cuda")
    X, nf = ops.als_solve_rows(_csr(rows, N_COLS), case.Y_dev * 0.01, G_bad, alpha=1.0, reg=0.5, out=out)
    assert int(nf.item()) == sum(1 for r in rows if len(r)) == 6
    assert not X.cpu().numpy().any()
    again, nf2 = ops.als_solve_rows(case.csr, case.Y_dev, case.G_dev, alpha=ALPHA, reg=REG)
    assert int(nf2.item()) == 0 and t.equal(again, case.X_dev)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = _CASES.get(16) or Case(16)
    for d, word in ((6, "multiple of 4"), (132, "4 .. 128")):
        with pytest.raises(ValueError, match=word):
            ops.als_solve_rows(c.csr, t.zeros(N_COLS, d, device="cuda"), t.zeros(d, d, device="cuda"), alpha=1.0, reg=1.0)
    with pytest.raises(ValueError, match="alpha"):
        ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev, alpha=-1.0, reg=1.0)
    with pytest.raises(ValueError, match="reg"):
        ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev, alpha=1.0, reg=0.0)
    with pytest.raises(ValueError, match="G must be"):
        ops.als_solve_rows(c.csr, c.Y_dev, t.zeros(8, 8, device="cuda"), alpha=1.0, reg=1.0)
    with pytest.raises(ValueError, match="one row per column"):
        ops.als_solve_rows(c.csr, c.Y_dev[:10], c.G_dev, alpha=1.0, reg=1.0)
    with pytest.raises(ValueError, match="out must be"):
        ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev, alpha=1.0, reg=1.0, out=t.zeros(3, 16, device="cuda"))
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_solve_rows(c.csr, c.Y_dev.cpu(), c.G_dev, alpha=1.0, reg=1.0)
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev.cpu(), alpha=1.0, reg=1.0)
    with pytest.raises(TypeError):
        ops.als_solve_rows(c.csr, c.Y_dev, c.G_dev, alpha=1.0, reg=1.0, row_list=t.zeros(2, dtype=t.int64, device="cuda"))
    # the C entry point on real device pointers: by return code, before anything is enqueued
    L = _lib.lib()
    nf = t.zeros(1, dtype=t.int32, device="cuda")
    X = t.full((N_ROWS, 16), 7.0, device="cuda")
    ws = t.empty(L.mi_als_solve_rows_workspace_bytes(N_ROWS, c.csr.nnz, 16), dtype=t.uint8, device="cuda")
    misaligned = c.Y_dev.contiguous().reshape(-1)[1:1 + 16 * (N_COLS - 1)].reshape(N_COLS - 1, 16)

    def call(d=16, Y=c.Y_dev, ldy=24, n_cols=N_COLS, nnz=c.csr.nnz, alpha=1.0, reg=1.0, ws_bytes=ws.numel()):
        return L.mi_als_solve_rows_f32(N_ROWS, d, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), nnz, n_cols, Y.data_ptr(), ldy,
                                       c.G_dev.data_ptr(), alpha, reg, X.data_ptr(), 16, None, 0, nf.data_ptr(), ws.data_ptr(),
                                       ws_bytes, ops._stream())
    bad = _lib.MI_ERR_BAD_ARG
    assert call(d=6) == bad and call(d=132) == bad and call(d=0) == bad
    assert call(n_cols=1 << 31) == bad and call(nnz=1 << 31) == bad
    assert call(Y=misaligned, ldy=16) == bad and call(ldy=18) == bad and call(ldy=12) == bad
    assert call(alpha=-1.0) == bad and call(reg=0.0) == bad
    assert call(ws_bytes=ws.numel() - 256) == _lib.MI_ERR_WORKSPACE
    t.cuda.synchronize()
    assert int(nf.item()) == 0 and bool((X == 7.0).all())             # nothing was enqueued


# ---- 6. the trainer -------------------------------------------------------------------------------------------------------------
def _small_graph():
    rng = np.random.default_rng(11)
    pairs = rng.choice(60 * 40, size=400, replace=False)
    return t.from_numpy(np.stack([pairs // 40, pairs % 40]).astype(np.int64))


def _bound_slack(ptr, idx, Yfix_dev, X, alpha, reg):
    """sum over rows of bound_r^2 / (2 reg): how far above the half-sweep's exact minimum its float32 rows may end
    (tests/als_emulation.py, "Objective slack"), with the derived residual bound in the residual's place.  The bound is taken
    for the system the kernel was given — G from the f32 GEMM, as the trainer forms it — and widened by that G's distance from
    the float64 Gram matrix of the objective, at most g(n) |Y|^T |Y| (an f32 chain over the n rows of Y, however it is split)."""
    Yfix = Yfix_dev.cpu().numpy()
    G = ops.gemm(Yfix_dev, Yfix_dev, trans_a=True, trans_b=False).cpu().numpy()
    G = np.tril(G) + np.tril(G, -1).T                                 # the kernel reads the lower triangle
    absY = np.abs(Yfix).astype(np.float64)
    extra = AE.g(Yfix.shape[0]) * np.linalg.norm(absY.T @ absY, "fro")
    total = 0.0
    for r in range(len(ptr) - 1):
        e = idx[ptr[r]:ptr[r + 1]]
        if len(e):
            b = AE.residual_bound(e, Yfix, G, alpha, reg, X[r]) + extra * np.linalg.norm(X[r].astype(np.float64))
            total += b * b
    return total / (2.0 * reg)


def test_trainer_objective_fit_and_fold_in():
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 40)
    alpha, reg = 1.0, 2.0
    model = ImplicitALS(60, 40, dim=16, alpha=alpha, reg=reg, seed=3).cuda()
    ptr_u, idx_u = AE.csr_of(ei[0].numpy(), ei[1].numpy(), 60)
    ptr_i, idx_i = AE.csr_of(ei[1].numpy(), ei[0].numpy(), 40)
    prev = model.objective(inter)
    want = AE.objective(ptr_u, idx_u, model.users_emb.weight.cpu().numpy(), model.items_emb.weight.cpu().numpy(), alpha, reg)
    assert abs(prev - want) <= 1e-9 * abs(want)                       # the device objective is the emulation's
    for epoch in range(3):
        for side in ("users", "items"):
            assert int(model.half_sweep(side, inter).item()) == 0
            Xd, Yd = model.users_emb.weight.data, model.items_emb.weight.data
            slack = (_bound_slack(ptr_u, idx_u, Yd, Xd.cpu().numpy(), alpha, reg) if side == "users"
                     else _bound_slack(ptr_i, idx_i, Xd, Yd.cpu().numpy(), alpha, reg))
            cur = model.objective(inter)
            print(f"epoch {epoch} {side}: objective {cur:.9g} (previous {prev:.9g}, slack {slack:.3e})")
            assert cur <= prev + slack
            prev = cur
            if side == "users":                                       # fold-in of a training user's own row: the same op
                csr = inter.csr()
                for u in (0, 17, 59):
                    lo, hi = int(csr.rowptr[u]), int(csr.rowptr[u + 1])
                    p = t.tensor([0, hi - lo], dtype=t.int32, device="cuda")
                    assert t.equal(model.fold_in(p, csr.col[lo:hi].contiguous())[0], model.users_emb.weight[u])
    a = ImplicitALS(60, 40, dim=16, alpha=alpha, reg=reg, seed=5).cuda().fit(inter, 3)
    b = ImplicitALS(60, 40, dim=16, alpha=alpha, reg=reg, seed=5).cuda().fit(Interactions(ei.cuda(), 60, 40), 3)
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    # the consumers of LightGCN's tables take the module
    users = t.arange(60, dtype=t.int64, device="cuda")
    top = topk_for_users(a.users_emb.weight.detach(), a.items_emb.weight.detach(), users, ei.cuda(), 5)
    assert top.shape == (60, 5)
    seen = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert not any((u, int(i)) in seen for u, row in enumerate(top.cpu().tolist()) for i in row)
    held = t.stack([users[:20], top[:20, 0]])                         # each user's best unseen item as a held-out pair: rank 0
    m = get_full_rank_metrics_lightgcn(a, held, [ei.cuda()], ks=(5,))
    assert m["recall@5"] == 1.0 and abs(m["mrr"] - 1.0) < 1e-12


def test_fit_raises_on_failed_rows():
    ei = _small_graph()
    model = ImplicitALS(60, 40, dim=16, alpha=1.0, reg=1.0, seed=0).cuda()
    model.items_emb.weight.fill_(float("nan"))                        # every user system has a NaN pivot: arithmetic, no fault
    with pytest.raises(RuntimeError, match="pivot"):
        model.fit(Interactions(ei.cuda(), 60, 40), 1)


def test_pipeline_writes_what_the_matcher_reads(tmp_path):
    """als.train: run_pipeline_lightgcn's split and evaluation with iALS in the trainer's place, and the three files
    data.matching.LightGCNMatcher consumes."""
    import json
    import math
    import os
    from dataclasses import replace
    from laplace_amd import als
    from laplace_amd.config import lightgcn_config
    spec = S.SyntheticSpec(300, 200, 6000, seed=4, communities=4, community_mix=0.85, deg_min=5)
    ei = S.generate(spec)
    cfg = replace(lightgcn_config, k=12, num_recommendations=64)
    stats = als.train(cfg, edge_index=ei, num_users=300, num_articles=200, dim=16, alpha=1.0, reg=5.0, epochs=3,
                      save_dir=str(tmp_path), verbose=False)
    for v in (stats.loss, stats.recall_val, stats.recall_test, stats.precision_val, stats.precision_test):
        assert math.isfinite(v)
    assert stats.recall_test > 0.0
    top = t.load(os.path.join(tmp_path, "lightgcn_output.pt"))
    ue = t.load(os.path.join(tmp_path, "users_emb_final_lightgcn.pt"))
    ie = t.load(os.path.join(tmp_path, "items_emb_final_lightgcn.pt"))
    assert top.shape == (300, 64) and ue.shape == (300, 16) and ie.shape == (200, 16)
    full = json.load(open(os.path.join(tmp_path, "full_rank_metrics.json")))
    assert {"map@12", "recall@100", "mrr"} <= set(full)


# ---- 7. quality -----------------------------------------------------------------------------------------------------------------
def test_planted_graph_beats_popularity():
    """tools/map_planted.py's default recipe (943 x 1 682 x 100 000, 8 communities, mix 0.85, seed 5), d = 64, alpha = 1,
    reg = 20, 5 epochs: map@12 of the held-out pairs above the popularity predictor's, both from full_rank_metrics.
    float64 numpy measures about 0.100 against 0.052 (tests/test_als_cpu.py)."""
    spec = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).cuda()
    inter = Interactions(ei.cuda(), spec.num_users, spec.num_items)
    model = ImplicitALS(spec.num_users, spec.num_items, dim=64, alpha=1.0, reg=20.0, seed=0).cuda().fit(inter, 5)
    m_als = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], ks=(12,))["map@12"]
    deg = t.bincount(inter.edge_index[1], minlength=spec.num_items).to(t.float32)
    ue = t.zeros(spec.num_users, 4, device="cuda")
    ue[:, 0] = 1.0
    ie = t.zeros(spec.num_items, 4, device="cuda")
    ie[:, 0] = deg
    m_pop = get_full_rank_metrics_lightgcn(None, held, [inter.edge_index], ks=(12,), embeddings=(ue, ie))["map@12"]
    print(f"map@12: iALS {m_als:.4f}, popularity {m_pop:.4f}")
    assert m_als > m_pop
