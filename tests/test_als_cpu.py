"""iALS without a GPU: the float64 statement of the rule (tests/als_emulation.py) is a minimiser of the objective it claims,
the accuracy bound holds for a float32 reference implementation and is not vacuous, the entry points refuse what the header
says they refuse, and the planted C1-scale recipe beats the popularity predictor."""
import numpy as np
import pytest
import torch as t

import als_emulation as AE
from laplace_amd import _lib, ops, synthetic as S


def _problem(d, n_rows=12, n_cols=40, seed=0, max_len=30, noise=0.1):
    rng = np.random.default_rng(seed)
    # a common offset in every factor row: G, S and b are then dominated by one direction, as trained factors are
    Y = (0.5 + rng.standard_normal((n_cols, d)) * noise).astype(np.float32)
    lens = rng.integers(1, max_len, n_rows)
    lens[0] = 0
    rows = [rng.integers(0, n_cols, n).tolist() for n in lens]
    G = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    G = np.maximum(G, G.T)
    return Y, G, rows


def test_float64_solution_zeroes_the_gradient():
    Y, G, rows = _problem(16)
    for e in rows[1:]:
        x = AE.x64(e, Y, G, 1.5, 0.75)
        grad = AE.objective_gradient_row(e, Y, G, 1.5, 0.75, x)
        A, b = AE.system64(e, Y, G, 1.5, 0.75)
        assert np.linalg.norm(grad) <= 1e-12 * (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))
    assert not AE.x64([], Y, G, 1.5, 0.75).any()


def test_gradient_is_the_objectives():
    """A x - b is the derivative of AE.objective in a row: central differences on the full objective."""
    rng = np.random.default_rng(1)
    U_, I_, d, alpha, reg = 5, 7, 4, 1.5, 0.75
    X, Y = rng.standard_normal((U_, d)), rng.standard_normal((I_, d)).astype(np.float32)
    ptr, idx = AE.csr_of([0, 0, 1, 2, 2, 2, 4], [1, 3, 0, 2, 2, 6, 5], U_)   # user 2 holds item 2 twice, user 3 nothing
    G = Y.astype(np.float64).T @ Y.astype(np.float64)
    for r in (0, 2, 3):
        e = idx[ptr[r]:ptr[r + 1]]
        A, b = AE.system64(e, Y, G, alpha, reg) if len(e) else (G + reg * np.eye(d), np.zeros(d))
        grad = A @ X[r] - b
        for j in range(d):
            h = 1e-5
            Xp, Xm = X.copy(), X.copy()
            Xp[r, j] += h
            Xm[r, j] -= h
            num = (AE.objective(ptr, idx, Xp, Y, alpha, reg) - AE.objective(ptr, idx, Xm, Y, alpha, reg)) / (2 * h)
            assert abs(num - grad[j]) <= 1e-6 * max(1.0, abs(grad[j]))


def test_objective_does_not_increase_over_float64_half_sweeps():
    rng = np.random.default_rng(2)
    U_, I_, d, alpha, reg = 30, 20, 8, 1.0, 2.0
    pairs = np.unique(rng.integers(0, U_ * I_, 200))
    u, i = pairs // I_, pairs % I_
    ptr_u, idx_u = AE.csr_of(u, i, U_)
    ptr_i, idx_i = AE.csr_of(i, u, I_)
    X, Y = rng.standard_normal((U_, d)) * 0.1, rng.standard_normal((I_, d)) * 0.1
    prev = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
    for _ in range(3):
        X = AE.half_sweep64(ptr_u, idx_u, Y, alpha, reg)
        cur = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
        assert cur <= prev * (1 + 1e-12)
        prev = cur
        Y = AE.half_sweep64(ptr_i, idx_i, X, alpha, reg)
        cur = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
        assert cur <= prev * (1 + 1e-12)
        prev = cur


@pytest.mark.parametrize("d", [4, 16, 64, 128])
def test_f32_reference_inside_the_bound_and_bound_not_vacuous(d):
    """A relative perturbation p of x moves the residual by p ||A x||, while the bound's solve term is about
    g(3 d) trace(A) ||x||: the bound can tell the two apart when ||A x|| / ||x|| is a fair share of trace(A), i.e. when b lies
    near A's dominant eigenvectors.  Factor rows with a common offset and little scatter, and the model's default reg, give
    such systems at every d (at d = 128 the perturbed residual is about 5 bounds; scattered rows at reg = 0.75 would leave it at
    0.8 of one: there a relative 1e-3 is within what float32 Cholesky may lose, and no rigorous bound could flag it)."""
    Y, G, rows = _problem(d, seed=d, noise=0.02)
    alpha, reg = 1.5, 20.0
    for e in rows[1:]:
        A32, b32 = AE.form_f32(e, Y, G, alpha, reg)
        x = AE.cholesky_solve_f32(A32, b32)
        assert x is not None
        res, bound = AE.residual(e, Y, G, alpha, reg, x), AE.residual_bound(e, Y, G, alpha, reg, x)
        assert res <= bound, (d, len(e), res, bound)
        bad = x.astype(np.float64) * (1.0 + 1e-3)   # b - A x' = r - 1e-3 A x: three orders above any float32 rounding
        assert AE.residual(e, Y, G, alpha, reg, bad) > AE.residual_bound(e, Y, G, alpha, reg, bad), (d, len(e))


def test_f32_reference_reports_a_bad_pivot():
    Y, G, rows = _problem(8)
    A32, b32 = AE.form_f32(rows[1], Y, -10.0 * np.eye(8, dtype=np.float32), 1.0, 0.5)
    assert AE.cholesky_solve_f32(A32, b32) is None


def test_check_als_names_the_constraint():
    ops.check_als(64, 1.0, 20.0)
    ops.check_als(4, 0.0, 1e-3)
    ops.check_als(128, 40, 1)
    for d, word in ((6, "multiple of 4"), (0, "4 .. 128"), (132, "4 .. 128"), (-4, "4 .. 128"), (64.0, "integer"), (True, "integer")):
        with pytest.raises(ValueError, match=word):
            ops.check_als(d, 1.0, 1.0)
    for alpha in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="alpha"):
            ops.check_als(64, alpha, 1.0)
    for reg in (0.0, -2.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="reg"):
            ops.check_als(64, 1.0, reg)


def test_entry_point_refuses_before_enqueueing():
    """Every refusal of mi_als_solve_rows_f32 comes back before a pointer is touched: made-up device addresses are enough."""
    L = _lib.lib()
    assert [L.mi_als_chunk(d) for d in (4, 64, 68, 128)] == [4096, 4096, 2048, 2048]
    assert [L.mi_als_chunk(d) for d in (0, 6, 132, -4)] == [0, 0, 0, 0]
    P, big = 0x10000, 1 << 31

    def call(n_rows=10, d=16, nnz=100, n_cols=50, Y=P, ldy=16, alpha=1.0, reg=1.0, ldx=16, row_list=None, n_list=0, nf=P, ws=P,
             ws_bytes=1 << 30):
        return L.mi_als_solve_rows_f32(n_rows, d, P, P, nnz, n_cols, Y, ldy, P, alpha, reg, P, ldx, row_list, n_list, nf, ws,
                                       ws_bytes, None)
    bad, short = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    assert call(d=6) == bad and call(d=0) == bad and call(d=132) == bad
    assert call(n_cols=big) == bad and call(nnz=big) == bad and call(n_rows=big) == bad
    assert call(n_rows=-1) == bad and call(nnz=-1) == bad and call(row_list=P, n_list=-1) == bad
    assert call(alpha=-0.5) == bad and call(alpha=float("nan")) == bad and call(reg=0.0) == bad and call(reg=float("inf")) == bad
    assert call(Y=P + 4) == bad and call(ldy=18) == bad and call(ldy=12) == bad and call(ldx=15) == bad
    assert call(Y=None) == bad and call(nf=None) == bad
    need = L.mi_als_solve_rows_workspace_bytes(10, 100, 16)
    assert need > 0 and call(ws_bytes=need - 1) == short and call(ws=None) == short
    assert call(n_rows=0) == 0 and call(row_list=P, n_list=0) == 0                    # nothing to do: nothing enqueued
    # the workspace: (d * d + d) * 4 bytes per possible chunk of a long row, 8 bytes per row, 256-byte granules
    chunk, nnz, d = 2048, 10_000_000, 128
    cap = nnz // chunk + nnz // (chunk + 1)
    got = L.mi_als_solve_rows_workspace_bytes(1000, nnz, d)
    assert cap * (d * d + d) * 4 <= got <= cap * (d * d + d) * 4 + cap * 4 + 1000 * 4 + 4 * 256
    assert L.mi_als_solve_rows_workspace_bytes(10, big, 16) == 0 and L.mi_als_solve_rows_workspace_bytes(10, 10, 6) == 0


def test_ops_refuse_cpu_tensors():
    ptr, idx = t.tensor([0, 2], dtype=t.int32), t.tensor([0, 1], dtype=t.int32)
    csr = ops.DeviceCSR(1, 2, ptr, idx)
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_solve_rows(csr, t.zeros(2, 4), t.eye(4), alpha=1.0, reg=1.0)


def test_planted_recipe_beats_popularity_in_float64():
    """tools/map_planted.py's default recipe, d = 64, alpha = 1, reg = 20, 5 epochs of float64 iALS: MAP@12 on the held-out
    pairs above the popularity predictor's on the same pairs (measured: about 0.100 against 0.052)."""
    spec = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).numpy()
    u, i = ei[0].numpy(), ei[1].numpy()
    ptr_u, idx_u = AE.csr_of(u, i, spec.num_users)
    ptr_i, idx_i = AE.csr_of(i, u, spec.num_items)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((spec.num_users, 64)) * 0.1
    Y = rng.standard_normal((spec.num_items, 64)) * 0.1
    for _ in range(5):
        X = AE.half_sweep64(ptr_u, idx_u, Y, 1.0, 20.0)
        Y = AE.half_sweep64(ptr_i, idx_i, X, 1.0, 20.0)
    m_als = AE.map_at_k_single(X[held[0]] @ Y.T, held[0], held[1], ptr_u, idx_u)
    deg = np.bincount(i, minlength=spec.num_items).astype(np.float64)
    m_pop = AE.map_at_k_single(np.broadcast_to(deg, (held.shape[1], spec.num_items)), held[0], held[1], ptr_u, idx_u)
    print(f"MAP@12 float64 iALS {m_als:.4f}, popularity {m_pop:.4f}")
    assert m_als > m_pop
