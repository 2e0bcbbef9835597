"""The iALS block solver without a GPU: the float64 statement of its rule (tests/als_block_emulation.py) is the block-wise
exact minimiser it claims, it keeps up with the full solver over epochs, the exact case is exact, the GPU test's tolerance
can tell a wrong schedule from the rule, and the entry points refuse what the header says they refuse."""
import numpy as np
import pytest
import torch as t

import als_block_cases as BC
import als_block_emulation as BE
import als_emulation as AE
from laplace_amd import _lib, ops, synthetic as S
from laplace_amd.als import ImplicitALS


def _problem(d, n_rows=10, n_cols=40, seed=0):
    rng = np.random.default_rng(seed)
    Y = (0.5 + rng.standard_normal((n_cols, d)) * 0.1).astype(np.float32)
    rows = [rng.integers(0, n_cols, n).tolist() for n in rng.integers(1, 30, n_rows)]
    G = BE.sym_lower((Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32))
    return Y, G, rows, rng.standard_normal((n_rows, d))


@pytest.mark.parametrize("d,B", [(16, 16), (24, 32), (40, 64), (64, 64)])
def test_one_block_equals_the_full_solve(d, B):
    Y, G, rows, X0 = _problem(d, seed=d)
    for r, e in enumerate(rows):
        want = AE.x64(e, Y, G, 1.5, 0.75)
        for x0 in (None, X0[r]):
            got = BE.block_sweep64(e, Y, G, 1.5, 0.75, x0, B, 1)
            assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want), (d, r)
    assert not BE.block_sweep64([], Y, G, 1.5, 0.75, X0[0], B, 1).any()      # an empty row is zero whatever its start


@pytest.mark.parametrize("d,B", [(40, 16), (64, 32), (32, 8)])
def test_row_share_never_rises_from_block_to_block(d, B):
    Y, G, rows, X0 = _problem(d, seed=100 + d)
    for r, e in enumerate(rows):
        vals = [BE.row_share64(e, Y, G, 1.5, 0.75, X0[r])]
        BE.block_sweep64(e, Y, G, 1.5, 0.75, X0[r], B, 3, hook=lambda x: vals.append(BE.row_share64(e, Y, G, 1.5, 0.75, x)))
        assert len(vals) == 1 + 3 * len(BE.blocks(d, B))
        for a, b in zip(vals, vals[1:]):
            assert b <= a + 1e-12 * max(1.0, abs(a)), (d, B, r)
        x_full = AE.x64(e, Y, G, 1.5, 0.75)
        assert vals[-1] >= BE.row_share64(e, Y, G, 1.5, 0.75, x_full) - 1e-9 * abs(vals[-1])


def test_epochs_against_the_full_solver():
    """Planted 400 x 300 graph, d = 32, alpha 1, reg 20, the same start: the objective never rises over block half-sweeps, and
    the block solver (B = 16, one sweep) after k + 1 epochs is not above the full float64 solver after k epochs, k = 1, 2
    (measured in float64 on this graph: full 7463.21 / 6071.07 after 1 / 2 epochs, block 7461.09 / 6107.55 / 6030.04 after
    1 / 2 / 3)."""
    spec = S.SyntheticSpec(400, 300, 8000, seed=3, communities=4, community_mix=0.85, deg_min=1)
    ei = S.generate(spec).numpy()
    ptr_u, idx_u = AE.csr_of(ei[0], ei[1], 400)
    ptr_i, idx_i = AE.csr_of(ei[1], ei[0], 300)
    rng = np.random.default_rng(0)
    d, alpha, reg = 32, 1.0, 20.0
    X0, Y0 = rng.standard_normal((400, d)) * 0.1, rng.standard_normal((300, d)) * 0.1
    X, Y, full = X0, Y0, []
    for _ in range(2):
        X = AE.half_sweep64(ptr_u, idx_u, Y, alpha, reg)
        Y = AE.half_sweep64(ptr_i, idx_i, X, alpha, reg)
        full.append(AE.objective(ptr_u, idx_u, X, Y, alpha, reg))
    X, Y, block = X0, Y0, []
    prev = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
    for _ in range(3):
        X = BE.half_sweep(BE.block_sweep64, ptr_u, idx_u, Y, Y.T @ Y, alpha, reg, X, 16, 1)
        mid = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
        Y = BE.half_sweep(BE.block_sweep64, ptr_i, idx_i, X, X.T @ X, alpha, reg, Y, 16, 1)
        cur = AE.objective(ptr_u, idx_u, X, Y, alpha, reg)
        assert mid <= prev * (1 + 1e-12) and cur <= mid * (1 + 1e-12)
        prev = cur
        block.append(cur)
    print("full", full, "block", block)
    assert block[1] <= full[0] and block[2] <= full[1]


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_case_is_exact_in_float32(sweeps, warm):
    Y, G, rows, X0 = BC.exact_case()
    moved = 0
    for r, e in enumerate(rows):
        x0 = X0[r] if warm else None
        x64 = BE.block_sweep64(e, Y, G, 1.0, 1.0, x0, 16, sweeps)
        x32 = BE.block_sweep_f32(e, Y, G, 1.0, 1.0, x0, 16, sweeps)
        assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64), x64), r
        if len(e):
            moved += int(np.abs(x64 - BE.block_sweep64(e, Y, G, 1.0, 1.0, x0, 16, sweeps + 1)).max() > 0)
    assert moved > 0          # the blocks couple: another sweep still moves some row, so this is no one-step problem


@pytest.mark.parametrize("d,B", [(40, 16), (64, 32), (128, 64), (256, 16)])
def test_the_gpu_tolerance_is_not_vacuous(d, B):
    """On the GPU test's inputs the Jacobi schedule — no update of p and x between the blocks of a sweep — is further from
    the rule than 8 times the float32 reference's error, the tolerance the kernel is held to."""
    pr = BC.problem(d, B)
    for from_zero, sweeps in ((True, 1), (False, 1)):
        X64, _, tol = pr.refs(from_zero, sweeps)
        jac = np.stack([BE.jacobi_sweep64(e, pr.Y, pr.G, BC.ALPHA, BC.REG, None if from_zero else pr.X0[r], B, sweeps)
                        for r, e in enumerate(pr.rows)])
        dev = np.linalg.norm(jac - X64, axis=1).max()
        print(f"d={d} B={B} from_zero={from_zero}: jacobi {dev:.3e}, tolerance {tol:.3e}")
        assert tol > 0 and dev > 10 * tol


def test_check_als_block_names_the_constraint():
    ops.check_als_block(256, 16, 1, 1.0, 20.0)
    ops.check_als_block(4, 64, 64, 0.0, 1e-3)
    for d, word in ((6, "multiple of 4"), (0, "4 .. 256"), (260, "4 .. 256"), (64.0, "integer"), (True, "integer")):
        with pytest.raises(ValueError, match=word):
            ops.check_als_block(d, 16, 1, 1.0, 1.0)
    for block in (8, 48, 128, 16.5, True, None):
        with pytest.raises(ValueError, match="block"):
            ops.check_als_block(64, block, 1, 1.0, 1.0)
    for sweeps in (0, 65, -1, 1.5, True):
        with pytest.raises(ValueError, match="sweeps"):
            ops.check_als_block(64, 16, sweeps, 1.0, 1.0)
    with pytest.raises(ValueError, match="alpha"):
        ops.check_als_block(64, 16, 1, -1.0, 1.0)
    with pytest.raises(ValueError, match="reg"):
        ops.check_als_block(64, 16, 1, 1.0, 0.0)


def test_trainer_keywords():
    m = ImplicitALS(6, 5, dim=256, solver="block", block=32, block_sweeps=2, fold_in_sweeps=8)
    assert (m.solver, m.block, m.block_sweeps, m.fold_in_sweeps) == ("block", 32, 2, 8)
    assert ImplicitALS(6, 5, dim=16).solver == "cholesky"
    with pytest.raises(ValueError, match='requires solver="block"'):
        ImplicitALS(6, 5, dim=256)
    with pytest.raises(ValueError, match="solver"):
        ImplicitALS(6, 5, dim=16, solver="cg")
    with pytest.raises(ValueError, match="4 .. 256"):
        ImplicitALS(6, 5, dim=260, solver="block")
    with pytest.raises(ValueError, match="block"):
        ImplicitALS(6, 5, dim=16, solver="block", block=8)
    with pytest.raises(ValueError, match="sweeps"):
        ImplicitALS(6, 5, dim=16, solver="block", fold_in_sweeps=0)


def test_entry_point_refuses_before_enqueueing():
    """Every refusal of mi_als_block_rows_f32 comes back before a pointer is touched: made-up device addresses are enough."""
    L = _lib.lib()
    for d in (4, 16, 40, 64, 128, 256):
        for B in (16, 32, 64):
            c = L.mi_als_block_chunk(d, B)
            assert c >= 4 and c == ops.als_block_chunk(d, B)
    assert [L.mi_als_block_chunk(d, B) for d, B in ((0, 16), (6, 16), (260, 16), (64, 8), (64, 48), (64, 128))] == [0] * 6
    P, big = 0x10000, 1 << 31

    def call(n_rows=10, d=16, block=16, sweeps=1, nnz=100, n_cols=50, Y=P, ldy=16, alpha=1.0, reg=1.0, ldx=16, from_zero=0,
             row_list=None, n_list=0, nf=P, ws=P, ws_bytes=1 << 30):
        return L.mi_als_block_rows_f32(n_rows, d, block, sweeps, P, P, nnz, n_cols, Y, ldy, P, alpha, reg, P, ldx, from_zero,
                                       row_list, n_list, nf, ws, ws_bytes, None)
    bad, short = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    assert call(d=6) == bad and call(d=0) == bad and call(d=260, ldy=260, ldx=260) == bad
    assert call(block=8) == bad and call(block=48) == bad and call(block=128) == bad
    assert call(sweeps=0) == bad and call(sweeps=65) == bad
    assert call(n_cols=big) == bad and call(nnz=big) == bad and call(n_rows=big) == bad
    assert call(n_rows=-1) == bad and call(nnz=-1) == bad and call(row_list=P, n_list=-1) == bad
    assert call(alpha=-0.5) == bad and call(alpha=float("nan")) == bad and call(reg=0.0) == bad and call(reg=float("inf")) == bad
    assert call(Y=P + 4) == bad and call(ldy=18) == bad and call(ldy=12) == bad and call(ldx=15) == bad
    assert call(Y=None) == bad and call(nf=None) == bad
    need = L.mi_als_block_rows_workspace_bytes(10, 100, 16, 16)
    assert need > 0 and call(ws_bytes=need - 1) == short and call(ws=None) == short
    assert call(n_rows=0) == 0 and call(row_list=P, n_list=0) == 0                    # nothing to do: nothing enqueued
    # the workspace: G as a full d x d matrix, and one float per entry (p_e of the rows that are not resident), each in
    # 256-byte granules, whatever B and the number of rows
    for nnz, want in ((0, 256), (1, 256), (64, 256), (65, 512), (10_000_000, 40_000_000)):
        assert L.mi_als_block_rows_workspace_bytes(1000, nnz, 256, 64) == 256 * 256 * 4 + want
        assert L.mi_als_block_rows_workspace_bytes(5, nnz, 16, 16) == 16 * 16 * 4 + want
        assert L.mi_als_block_rows_workspace_bytes(5, nnz, 4, 32) == 256 + want
    assert L.mi_als_block_rows_workspace_bytes(10, big, 16, 16) == 0 and L.mi_als_block_rows_workspace_bytes(10, 10, 6, 16) == 0
    assert L.mi_als_block_rows_workspace_bytes(10, 10, 16, 8) == 0 and L.mi_als_block_rows_workspace_bytes(-1, 10, 16, 16) == 0


def test_ops_refuse_cpu_tensors():
    ptr, idx = t.tensor([0, 2], dtype=t.int32), t.tensor([0, 1], dtype=t.int32)
    csr = ops.DeviceCSR(1, 2, ptr, idx)
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_block_rows(csr, t.zeros(2, 4), t.eye(4), alpha=1.0, reg=1.0)
