"""The hub path of the iALS block solver without a GPU: the float64 statement of its rule (tests/als_hub_emulation.py) is the
block rule's own iteration, its float32 statement stays inside the yardstick the kernel is held to (8 times the committed
float32 block reference's distance from float64) while a wrong schedule does not, the exact case is exact, and the keyword
and the C entries refuse what the header says they refuse."""
import numpy as np
import pytest

import als_block_cases as BC
import als_block_emulation as BE
import als_hub_cases as HC
import als_hub_emulation as HE
import als_weighted_emulation as WE
from laplace_amd import _lib, ops
from laplace_amd.als import ImplicitALS

ALPHA, REG = HC.ALPHA, HC.REG
CPU_STARTS = ((True, 1), (False, 3))


@pytest.mark.parametrize("d,B", HC.SHAPES)
def test_float64_hub_form_is_the_block_rule(d, B):
    pr = HC.problem(d, B)
    worst = 0.0
    for from_zero, sweeps in BC.STARTS:
        for r, e in enumerate(pr.rows):
            x0 = None if from_zero else pr.X0[r]
            want = BE.block_sweep64(e, pr.Y, pr.G, ALPHA, REG, x0, B, sweeps)
            got = HE.hub_sweep64(e, pr.Y, pr.G, ALPHA, REG, x0, B, sweeps)
            if len(e) == 0:
                assert not got.any()
                continue
            worst = max(worst, np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"d={d} B={B}: hub float64 against block float64, worst relative distance {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("d,B", HC.W_SHAPES)
def test_float64_weighted_hub_form_is_the_weighted_block_rule(d, B):
    pr = HC.weighted_problem(d, B)
    worst = 0.0
    for from_zero, sweeps in BC.STARTS:
        for r, e in enumerate(pr.rows):
            if len(e) == 0:
                continue
            x0 = None if from_zero else pr.X0[r]
            want = WE.block_sweep64(e, pr.conf[r], pr.Y, pr.G, pr.reg_rows[r], x0, B, sweeps)
            got = HE.hub_sweep64(e, pr.Y, pr.G, 0.0, pr.reg_rows[r], x0, B, sweeps, conf=pr.conf[r])
            worst = max(worst, np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"d={d} B={B}: weighted hub float64 against weighted block float64, worst relative distance {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("d,B", HC.SHAPES)
def test_float32_hub_form_inside_the_yardstick_and_jacobi_outside(d, B):
    """On the GPU test's inputs: max_r ||x_hub_f32 - x_64|| <= 8 max_r ||x_block_f32ref - x_64|| over the hub rows, and the
    Jacobi schedule of the hub form (every block of a sweep from the sweep's start) is outside it."""
    pr = HC.problem(d, B)
    rows = pr.hub_rows(4)
    for from_zero, sweeps in CPU_STARTS:
        X64, err32 = pr.refs(from_zero, sweeps)
        tol = 8.0 * err32[rows].max()
        hub = np.array([np.linalg.norm(HE.hub_sweep_f32(pr.rows[r], pr.Y, pr.G, ALPHA, REG, None if from_zero else pr.X0[r], B,
                                                        sweeps, pr.L).astype(np.float64) - X64[r]) for r in rows])
        jac = np.array([np.linalg.norm(HE.hub_jacobi64(pr.rows[r], pr.Y, pr.G, ALPHA, REG, None if from_zero else pr.X0[r], B,
                                                       sweeps) - X64[r]) for r in rows])
        print(f"RATIO d={d} B={B} from_zero={from_zero} sweeps={sweeps}: hub float32 {hub.max():.3e} block float32 reference "
              f"{tol / 8:.3e} ratio {hub.max() / (tol / 8):.2f}; jacobi {jac.max():.3e} = {jac.max() / tol:.1f} tolerances")
        assert tol > 0 and hub.max() <= tol
        if d > B:                                   # one block: Jacobi and Gauss-Seidel are the same schedule
            assert jac.max() > tol


@pytest.mark.parametrize("d,B", HC.W_SHAPES)
def test_float32_weighted_hub_form_inside_the_yardstick(d, B):
    pr = HC.weighted_problem(d, B)
    rows = pr.hub_rows(4)
    for from_zero, sweeps in CPU_STARTS:
        X64, err32 = pr.refs_w(from_zero, sweeps, True)
        tol = 8.0 * err32[rows].max()
        hub = np.array([np.linalg.norm(HE.hub_sweep_f32(pr.rows[r], pr.Y, pr.G, 0.0, pr.reg_rows[r], None if from_zero else
                                                        pr.X0[r], B, sweeps, pr.L, conf=pr.conf[r]).astype(np.float64) - X64[r])
                        for r in rows])
        print(f"RATIO weighted d={d} B={B} from_zero={from_zero} sweeps={sweeps}: hub float32 {hub.max():.3e} block float32 "
              f"reference {tol / 8:.3e} ratio {hub.max() / (tol / 8):.2f}")
        assert tol > 0 and hub.max() <= tol


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_case_is_exact_in_float32(sweeps, warm):
    """als_block_cases.exact_case with every row of more than 2 entries a hub row: every operation of the hub rule is exact in
    float32 there as well, and the result is the block rule's, bit for bit."""
    Y, G, rows, X0 = BC.exact_case()
    n_hub = 0
    for r, e in enumerate(rows):
        if len(e) <= 2:
            continue
        n_hub += 1
        x0 = X0[r] if warm else None
        x64 = HE.hub_sweep64(e, Y, G, 1.0, 1.0, x0, 16, sweeps)
        x32 = HE.hub_sweep_f32(e, Y, G, 1.0, 1.0, x0, 16, sweeps, 4)         # chunks of 4 entries: several per row
        assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64), x64), r
        assert np.array_equal(x64, BE.block_sweep64(e, Y, G, 1.0, 1.0, x0, 16, sweeps)), r
    assert n_hub >= 8


def test_chunks_are_chains_of_their_own():
    """The float32 formation depends on the chunk length (so the constant is part of the rule) and not on the panel width."""
    pr = HC.problem(40, 16)
    e = pr.rows[6]                                                           # 70 entries
    A1, b1 = HE.form_f32(e, pr.Y, pr.G, ALPHA, REG, 4096)
    A2, b2 = HE.form_f32(e, pr.Y, pr.G, ALPHA, REG, 16)
    A3, b3 = HE.form_f32(e, pr.Y, pr.G, ALPHA, REG, 4096, panel=8)
    assert np.array_equal(A1, A3) and np.array_equal(b1, b3) and np.array_equal(A1, A1.T)
    assert not np.array_equal(A1, A2)
    A64, b64 = HE.system64(e, pr.Y, pr.G, ALPHA, REG)
    assert np.abs(A1 - A64).max() <= 1e-5 * np.abs(A64).max() and np.abs(b2 - b64).max() <= 1e-5 * np.abs(b64).max()


def test_hub_threshold_names_the_argument():
    ops.check_als_hub_threshold(None)
    ops.check_als_hub_threshold(None, "cholesky")
    ops.check_als_hub_threshold(1)
    ops.check_als_hub_threshold(1 << 40)
    for bad in (True, False, 0, -3, 2.0, "4", 1.5):
        with pytest.raises(ValueError, match="hub_threshold"):
            ops.check_als_hub_threshold(bad)
    with pytest.raises(ValueError, match="hub_threshold"):
        ops.check_als_hub_threshold(4, "cholesky")
    m = ImplicitALS(6, 5, dim=256, solver="block", hub_threshold=64)
    assert m.hub_threshold == 64 and ImplicitALS(6, 5, dim=16).hub_threshold is None
    for kw in (dict(solver="block", hub_threshold=0), dict(solver="block", hub_threshold=True),
               dict(solver="block", hub_threshold=8.0), dict(solver="cholesky", hub_threshold=8), dict(hub_threshold=8)):
        with pytest.raises(ValueError, match="hub_threshold"):
            ImplicitALS(6, 5, dim=16, **kw)


def test_hub_entries_refuse_before_enqueueing():
    """Every refusal of the hub entries comes back before a pointer is touched: made-up device addresses are enough."""
    L = _lib.lib()
    assert [L.mi_als_block_hub_chunk(d) for d in (4, 16, 64, 68, 128, 132, 256)] == [256, 256, 256, 512, 512, 512, 512]
    assert [L.mi_als_block_hub_chunk(d) for d in (0, 6, 260)] == [0, 0, 0]
    assert ops.als_block_hub_chunk(256) == 512
    P, big = 0x10000, 1 << 31

    def call(w=False, n_rows=10, d=16, block=16, sweeps=1, nnz=100, ldy=16, alpha=1.0, reg=1.0, thr=4, hr=3, hc=5, nf=P, ws=P,
             ws_bytes=1 << 30, conf=P):
        if w:
            return L.mi_als_block_rows_hub_w_f32(n_rows, d, block, sweeps, P, P, nnz, 50, P, ldy, P, conf, None, reg, P, 16, 0,
                                                 None, 0, thr, hr, hc, nf, ws, ws_bytes, None)
        return L.mi_als_block_rows_hub_f32(n_rows, d, block, sweeps, P, P, nnz, 50, P, ldy, P, alpha, reg, P, 16, 0, None, 0,
                                           thr, hr, hc, nf, ws, ws_bytes, None)
    bad, short = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    for w in (False, True):
        assert call(w, thr=0) == bad and call(w, thr=-1) == bad and call(w, thr=big) == bad
        assert call(w, hr=-1) == bad and call(w, hc=-1) == bad and call(w, hr=big) == bad and call(w, hc=big) == bad
        assert call(w, d=6) == bad and call(w, block=8) == bad and call(w, sweeps=0) == bad and call(w, nnz=big) == bad
        assert call(w, reg=0.0) == bad and call(w, ldy=18) == bad and call(w, nf=None) == bad
        assert call(w, n_rows=0) == 0                                      # nothing to do: nothing enqueued
        query = L.mi_als_block_rows_hub_w_workspace_bytes if w else L.mi_als_block_rows_hub_workspace_bytes
        need = query(10, 100, 16, 16, 3, 5)
        assert need > 0 and call(w, ws_bytes=need - 1) == short and call(w, ws=None) == short
    assert call(alpha=-1.0) == bad and call(True, conf=None) == bad
    # the formula of the header: the block entry's bytes, 256 for the counters, 4 per work row, 8 per hub row, 4 per chunk, a
    # chunk slot of the lower-triangle tiles and s, a row slot of d * d + d floats; every term in 256-byte granules
    q, base = L.mi_als_block_rows_hub_workspace_bytes, L.mi_als_block_rows_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    for d, n_work, nnz, hr, hc in ((16, 10, 100, 3, 5), (256, 1000, 10_000_000, 7, 450), (40, 5, 64, 0, 0), (128, 77, 999, 1, 1)):
        td = (d + 15) // 16
        slot = td * (td + 1) // 2 * 256 + 16 * td
        want = base(n_work, nnz, d, 16) + 256 + up(4 * n_work) + 2 * up(4 * hr) + up(4 * hc) + up(4 * hc * slot) + \
            up(4 * hr * (d * d + d))
        assert q(n_work, nnz, d, 16, hr, hc) == want == L.mi_als_block_rows_hub_w_workspace_bytes(n_work, nnz, d, 64, hr, hc)
    assert q(10, 100, 16, 16, -1, 0) == 0 and q(10, 100, 16, 16, 0, big) == 0 and q(10, 100, 6, 16, 1, 1) == 0
    assert q(-1, 100, 16, 16, 1, 1) == 0 and q(10, big, 16, 16, 1, 1) == 0 and q(10, 100, 16, 8, 1, 1) == 0
