"""No GPU: the weighted iALS rules as tests/als_weighted_emulation.py states them — agreement with the unweighted mirrors at
constant weights, the float32 references inside the derived bound on every problem of tests/test_gpu_als_weighted.py, the
vanishing gradient, the exact cases, the model's per-row regulariser, and every ValueError of the Python surface."""
import numpy as np
import pytest
import torch as t

import als_block_emulation as BE
import als_emulation as AE
import als_weighted_cases as WC
import als_weighted_emulation as WE
from laplace_amd import _lib, als, ops
from laplace_amd.interactions import Interactions

F = np.float32


# ---- 1. constant weights are the unweighted rule --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WC.CHOL_DIMS)
def test_constant_weights_equal_the_unweighted_float64_solution(d):
    pr = WC.chol_problem(d)
    for r, e in enumerate(pr.rows):
        a = np.full(len(e), WC.ALPHA, dtype=F)
        want = AE.x64(e, pr.Y, pr.G, WC.ALPHA, WC.REG)
        got = WE.x64(e, a, pr.Y, pr.G, WC.REG)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (d, r)


@pytest.mark.parametrize("d,B", WC.BLOCK_SHAPES)
def test_constant_weights_equal_the_unweighted_block_sweep(d, B):
    pr = WC.block_problem(d, B)
    for r, e in enumerate(pr.rows):
        a = np.full(len(e), WC.ALPHA, dtype=F)
        for from_zero, sweeps in WC.STARTS:
            x0 = None if from_zero else pr.X0[r]
            want = BE.block_sweep64(e, pr.Y, pr.G, WC.ALPHA, WC.REG, x0, B, sweeps)
            got = WE.block_sweep64(e, a, pr.Y, pr.G, WC.REG, x0, B, sweeps)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (d, B, r)


# ---- 2. the float32 reference meets the derived bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", WC.CHOL_DIMS)
def test_float32_reference_inside_the_bound(d):
    pr = WC.chol_problem(d)
    lens = [len(e) for e in pr.rows]
    assert lens[:7] == [0, 1, 3, 33, pr.L - 1, pr.L + 1, 2 * pr.L + 5]
    assert len(set(pr.rows[WC.REPEAT_ROW])) < len(pr.rows[WC.REPEAT_ROW]) and (pr.conf[WC.ZERO_ROW] == 0).sum() == 4
    for a in pr.conf:
        assert a.dtype == F and (len(a) == 0 or (a.min() >= 0 and a.max() <= 90.0))
    assert pr.reg_rows.min() >= 0.5 and pr.reg_rows.max() <= 5.0
    for r, x in enumerate(pr.x32()):
        assert x is not None
        pr.check_row(r, x, tag="f32ref ")


@pytest.mark.parametrize("d,B", WC.ONE_BLOCK_SHAPES)
def test_float32_block_reference_with_one_block_inside_the_bound(d, B):
    pr = WC.block_problem(d, B)
    for r, (e, a) in enumerate(zip(pr.rows, pr.conf)):
        x = WE.block_sweep_f32(e, a, pr.Y, pr.G, pr.reg_rows[r], None, B, 1)
        if len(e) == 0:
            assert not x.any()
            continue
        res, bound = WE.residual(e, a, pr.Y, pr.G, pr.reg_rows[r], x), WE.residual_bound(e, a, pr.Y, pr.G, pr.reg_rows[r], x)
        assert res <= bound, (d, B, r, res, bound)


def test_the_bound_tells_a_wrong_weight_from_the_rule():
    """A solution computed with one a_e doubled is outside the bound of the true weights: the bound is not vacuous."""
    pr = WC.chol_problem(16)
    for r in (2, 3, WC.REPEAT_ROW):
        e, a = pr.rows[r], pr.conf[r].copy()
        a[0] *= 2
        x = WE.x64(e, a, pr.Y, pr.G, pr.reg_rows[r])
        assert WE.residual(e, pr.conf[r], pr.Y, pr.G, pr.reg_rows[r], x) > WE.residual_bound(e, pr.conf[r], pr.Y, pr.G, pr.reg_rows[r], x)


# ---- 3. the gradient of the weighted objective ----------------------------------------------------------------------------------
def test_gradient_vanishes_at_the_float64_solution_and_matches_the_objective():
    pr = WC.chol_problem(16)
    rows, conf = pr.rows[:4] + pr.rows[7:], pr.conf[:4] + pr.conf[7:]
    reg_u = np.concatenate([pr.reg_rows[:4], pr.reg_rows[7:]]).astype(np.float64)
    Y = pr.Y.astype(np.float64)
    G = Y.T @ Y
    X = np.stack([WE.x64(e, a, pr.Y, G, reg_u[r]) for r, (e, a) in enumerate(zip(rows, conf))])
    for r, (e, a) in enumerate(zip(rows, conf)):
        if len(e):
            grad = WE.objective_gradient_row(e, a, pr.Y, G, reg_u[r], X[r])
            assert np.abs(grad).max() <= 1e-9 * max(1.0, np.abs(WE.system64(e, a, pr.Y, G, reg_u[r])[1]).max())
    # A x - b IS the derivative of the objective: a central difference along a random direction, row 3
    ptr, idx, cf = WC.csr_arrays(rows, conf)
    reg_i = np.full(WC.N_COLS, 0.7)
    rng = np.random.default_rng(0)
    X1 = X + rng.standard_normal(X.shape) * 0.05
    dirn = rng.standard_normal(16)
    h = 1e-5
    Xp, Xm = X1.copy(), X1.copy()
    Xp[3] += h * dirn
    Xm[3] -= h * dirn
    fd = (WE.objective(ptr, idx, cf, Xp, Y, reg_u, reg_i) - WE.objective(ptr, idx, cf, Xm, Y, reg_u, reg_i)) / (2 * h)
    want = WE.objective_gradient_row(rows[3], conf[3], pr.Y, G, reg_u[3], X1[3]) @ dirn
    assert abs(fd - want) <= 1e-6 * max(1.0, abs(want))


def test_constant_weights_objective_is_the_unweighted_objective():
    pr = WC.chol_problem(16)
    rows = pr.rows[:4] + pr.rows[7:]
    ptr, idx, _ = WC.csr_arrays(rows, [np.zeros(len(e), dtype=F) for e in rows])
    rng = np.random.default_rng(1)
    X = rng.standard_normal((len(rows), 16)) * 0.1
    got = WE.objective(ptr, idx, np.full(len(idx), WC.ALPHA, dtype=F), X, pr.Y, float(F(WC.REG)), float(F(WC.REG)))
    want = AE.objective(ptr, idx, X, pr.Y, WC.ALPHA, WC.REG)
    assert abs(got - want) <= 1e-12 * abs(want)


# ---- 4. the exact cases ---------------------------------------------------------------------------------------------------------
def test_exact_cholesky_case_is_exact_in_float32():
    Y, G, rows, conf, reg_rows = WC.exact_chol_case()
    assert len({float(a) for c in conf for a in c}) == 3
    for r, (e, a) in enumerate(zip(rows, conf)):
        x64, x32 = WE.x64(e, a, Y, G, reg_rows[r]), WE.x_f32(e, a, Y, G, reg_rows[r])
        assert np.array_equal(x32.astype(np.float64), x64), r
        A, _ = WE.system64(e, a, Y, G, reg_rows[r]) if len(e) else (np.eye(16) * 4, None)
        assert np.array_equal(A, np.diag(np.diag(A))) and np.all(np.log2(np.diag(A)) % 2 == 0)


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_block_case_is_exact_in_float32(sweeps, warm):
    Y, G, rows, conf, reg_rows, X0 = WC.exact_block_case()
    moved = False
    for r, (e, a) in enumerate(zip(rows, conf)):
        x0 = X0[r] if warm else None
        x64 = WE.block_sweep64(e, a, Y, G, reg_rows[r], x0, 16, sweeps)
        x32 = WE.block_sweep_f32(e, a, Y, G, reg_rows[r], x0, 16, sweeps)
        assert np.array_equal(x32.astype(np.float64), x64), r
        moved = moved or bool(x64.any())
    assert moved


# ---- 5. the model's regulariser -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [0.0, 0.5, 1.0])
def test_reg_rows_of_equals_the_float64_formula(nu):
    pr = WC.chol_problem(16)
    ptr, _, cf = WC.csr_arrays(pr.rows, pr.conf)
    got = als.reg_rows_of(t.from_numpy(ptr), t.from_numpy(cf), WC.N_COLS, 0.03, nu)
    want = WE.reg_rows64(ptr, cf, WC.N_COLS, 0.03, nu)
    assert got.dtype == t.float32 and got.shape == (len(pr.rows),)
    np.testing.assert_allclose(got.numpy().astype(np.float64), want, rtol=1e-6, atol=0)
    assert want[0] == pytest.approx(0.03 * WC.N_COLS ** nu)      # the empty row: the fixed table's own mass


def test_edge_confidence_is_alpha_times_the_weight_rounded_once():
    w = t.tensor([0.0, 1.0, 3.0, 0.1], dtype=t.float64)
    got = als.edge_confidence(w, 4, 1.7)
    assert got.dtype == t.float32 and t.equal(got, (w * 1.7).to(t.float32))


# ---- 6. every ValueError, without a device --------------------------------------------------------------------------------------
def test_ops_refuse_bad_weights_without_a_device():
    csr = ops.DeviceCSR(3, 5, t.tensor([0, 2, 2, 4], dtype=t.int32), t.tensor([0, 1, 2, 3], dtype=t.int32))
    Y, G = t.zeros(5, 16), t.zeros(16, 16)
    good_c, good_r = t.ones(4), t.ones(3)
    for fn in (ops.als_solve_rows, ops.als_block_rows):
        with pytest.raises(ValueError, match=r"conf must be a float32 tensor \[nnz\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=good_c.double())
        with pytest.raises(ValueError, match=r"conf must be a float32 tensor \[nnz\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=[1.0] * 4)
        with pytest.raises(ValueError, match=r"conf must have shape \[nnz\] = \[4\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=t.ones(5))
        with pytest.raises(ValueError, match=r"conf must have shape \[nnz\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=t.ones(2, 2))
        with pytest.raises(ValueError, match=r"reg_rows must be a float32 tensor \[n_rows\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=good_c, reg_rows=good_r.to(t.float16))
        with pytest.raises(ValueError, match=r"reg_rows must have shape \[n_rows\] = \[3\]"):
            fn(csr, Y, G, alpha=1.0, reg=1.0, reg_rows=t.ones(4))
        with pytest.raises(_lib.MiError, match="no CPU fallback"):     # well-formed weights: on to the device checks
            fn(csr, Y, G, alpha=1.0, reg=1.0, conf=good_c, reg_rows=good_r)
    ops.check_als_weights(4, 3, None, None)
    ops.check_als_weights(4, 3, good_c, good_r)


def test_model_refuses_bad_keywords_without_a_device():
    for bad in (-0.1, 1.5, float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="reg_power"):
            als.ImplicitALS(6, 5, dim=16, reg_power=bad)
    assert als.ImplicitALS(6, 5, dim=16).reg_power == 0.0 and als.ImplicitALS(6, 5, dim=16, reg_power=1).reg_power == 1.0
    ei = t.tensor([[0, 1, 2, 5], [4, 0, 1, 1]])
    inter = Interactions(ei, 6, 5)
    model = als.ImplicitALS(6, 5, dim=16)
    for bad, word in ((t.ones(3), "one weight per edge"), (t.ones(4, 1), "one weight per edge"),
                      (t.ones(4, dtype=t.int64), "floating-point"), ([1.0] * 4, "floating-point"),
                      (t.tensor([1.0, -0.5, 1.0, 1.0]), "finite and >= 0"),
                      (t.tensor([1.0, float("nan"), 1.0, 1.0]), "finite and >= 0"),
                      (t.tensor([1.0, float("inf"), 1.0, 1.0]), "finite and >= 0")):
        with pytest.raises(ValueError, match=word):
            model.bind(inter, bad)
        with pytest.raises(ValueError, match=word):
            model.fit(inter, 1, confidence=bad)
        with pytest.raises(ValueError, match=word):
            model.fold_in(t.tensor([0, 4], dtype=t.int32), t.tensor([0, 1, 2, 3], dtype=t.int32), confidence=bad)
    assert model._bound is None


def test_c_entries_refuse_before_touching_a_pointer():
    """Every refusal of the two weighted entries comes back before a pointer is touched: made-up addresses are enough."""
    L = _lib.lib()
    P = 0x1000
    bad = _lib.MI_ERR_BAD_ARG
    assert L.mi_als_solve_rows_w_workspace_bytes(7, 100, 16) == L.mi_als_solve_rows_workspace_bytes(7, 100, 16) > 0
    assert L.mi_als_block_rows_w_workspace_bytes(7, 100, 16, 16) == L.mi_als_block_rows_workspace_bytes(7, 100, 16, 16) > 0
    assert L.mi_als_solve_rows_w_workspace_bytes(7, 100, 6) == 0 and L.mi_als_block_rows_w_workspace_bytes(7, 100, 16, 8) == 0

    def chol(d=16, conf=P, reg_rows=None, reg=1.0, ldy=16, nnz=100, ws=P, ws_bytes=1 << 30, n_failed=P):
        return L.mi_als_solve_rows_w_f32(7, d, P, P, nnz, 50, P, ldy, P, conf, reg_rows, reg, P, 16, None, 0, n_failed, ws,
                                         ws_bytes, None)

    def block(d=16, B=16, sweeps=1, conf=P, reg_rows=None, reg=1.0, ldy=16, nnz=100, ws=P, ws_bytes=1 << 30):
        return L.mi_als_block_rows_w_f32(7, d, B, sweeps, P, P, nnz, 50, P, ldy, P, conf, reg_rows, reg, P, 16, 1, None, 0, P,
                                         ws, ws_bytes, None)
    for call in (chol, block):
        assert call(conf=None) == bad
        assert call(reg=0.0) == bad and call(reg=-1.0) == bad and call(reg=float("inf")) == bad and call(reg=float("nan")) == bad
        assert call(d=6) == bad and call(d=260) == bad and call(ldy=18) == bad and call(ldy=12) == bad and call(nnz=1 << 31) == bad
        assert call(ws=None) == _lib.MI_ERR_WORKSPACE and call(ws_bytes=16) == _lib.MI_ERR_WORKSPACE
        assert call(reg_rows=P, reg=0.0, ws_bytes=16) == _lib.MI_ERR_WORKSPACE      # reg is not looked at with reg_rows given
    assert chol(d=132) == bad and chol(n_failed=None) == bad
    assert block(B=8) == bad and block(sweeps=0) == bad and block(sweeps=65) == bad
