"""GPU: the iALS block row solver (mi_als_block_rows_f32, csrc/als_block.hip) against the float64 statement of its rule
(tests/als_block_emulation.py): inside the derived bound where one block is the whole row, within 8 times the float32
reference's own distance where there are several, an exact case, determinism and row purity across the resident and the
streaming path, failed pivots, refusals, and als.ImplicitALS(solver="block") end to end."""
import numpy as np
import pytest
import torch as t

import als_block_cases as BC
import als_block_emulation as BE
import als_emulation as AE
from laplace_amd import _lib, ops, synthetic as S
from laplace_amd.als import ImplicitALS
from laplace_amd.interactions import Interactions
from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn, topk_for_users

pytestmark = pytest.mark.gpu

ALPHA, REG, N_COLS, N_ROWS = BC.ALPHA, BC.REG, BC.N_COLS, BC.N_ROWS
SHAPES = [(d, B) for d in BC.DIMS for B in BC.BLOCKS]
ROW_LIST = [BC.LONG_ROW, 3, 39, 0, 6, 5, 1, 4]   # the long row, B - 1, a short one, the empty one, 70, 33, 1, B + 1


def _dev(a, dtype=None):
    x = t.from_numpy(np.ascontiguousarray(a)).cuda()
    return x if dtype is None else x.to(dtype)


def _csr(rows, n_cols):
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ops.DeviceCSR(len(rows), n_cols, _dev(ptr), _dev(idx))


class Case:
    """The device side of one BC.Problem: the operands and one batched call per start, shared by the tests below."""

    def __init__(self, d, B):
        self.pr = BC.problem(d, B)
        self.d, self.B = d, B
        self.Y_dev = _dev(self.pr.wide)[:, 4:4 + d]
        self.G_dev = _dev(self.pr.G)
        self.X0_dev = _dev(self.pr.X0)
        self.csr = _csr(self.pr.rows, N_COLS)
        self._out = {}

    def call(self, from_zero, sweeps, csr=None, rows=None, row_list=None):
        x = None
        if not from_zero:
            x = self.X0_dev.clone() if rows is None else self.X0_dev[rows].clone()
        return ops.als_block_rows(csr or self.csr, self.Y_dev, self.G_dev, alpha=ALPHA, reg=REG, block=self.B, sweeps=sweeps,
                                  x=x, row_list=row_list)

    def out(self, from_zero, sweeps):
        if (from_zero, sweeps) not in self._out:
            X, nf = self.call(from_zero, sweeps)
            assert int(nf.item()) == 0
            self._out[(from_zero, sweeps)] = X
        return self._out[(from_zero, sweeps)]


_CASES = {}


@pytest.fixture(params=SHAPES, ids=lambda s: f"d{s[0]}-B{s[1]}")
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(*request.param)
    return _CASES[request.param]


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,B", [(d, B) for d, B in SHAPES if d <= B])
def test_one_block_inside_the_derived_bound(d, B):
    """d <= B, a zero start, one sweep: the one block step solves the existing rule's A x = b, and the formation makes the
    roundings that als_emulation.residual_bound assumes (counted in tests/als_block_emulation.py)."""
    c = _CASES.setdefault((d, B), Case(d, B))
    assert c.Y_dev.stride(0) == d + 8
    X = c.out(True, 1).cpu().numpy()
    for r, e in enumerate(c.pr.rows):
        if len(e) == 0:
            assert not X[r].any()
            continue
        res, bound = AE.residual(e, c.pr.Y, c.pr.G, ALPHA, REG, X[r]), AE.residual_bound(e, c.pr.Y, c.pr.G, ALPHA, REG, X[r])
        print(f"d={d} B={B} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert np.isfinite(X[r]).all() and res <= bound, (d, B, r, res, bound)


@pytest.mark.parametrize("from_zero,sweeps", BC.STARTS)
def test_within_eight_times_the_float32_reference(case, from_zero, sweeps):
    """max_r ||x_kernel - x_64||_2 <= 8 * max_r ||x_f32ref - x_64||_2: the yardstick is the committed float32 reference on the
    same inputs; the factor covers another equally valid order of the same sums and fma against separate roundings."""
    X64, _, tol = case.pr.refs(from_zero, sweeps)
    X = case.out(from_zero, sweeps).cpu().numpy().astype(np.float64)
    assert np.isfinite(X).all() and not X[0].any()
    err = np.linalg.norm(X - X64, axis=1)
    print(f"RATIO d={case.d} B={case.B} from_zero={from_zero} sweeps={sweeps}: kernel {err.max():.3e} f32ref {tol / 8:.3e} "
          f"ratio {err.max() / (tol / 8):.2f} (long row {err[BC.LONG_ROW]:.3e})")
    assert tol > 0 and err.max() <= tol and err[BC.LONG_ROW] <= tol


# ---- 2. an exact case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_exact_case(sweeps, warm):
    """tests/als_block_cases.exact_case: every float32 operation of the rule is exact there (test_als_block_cpu.py asserts
    that the float32 and the float64 emulation agree bit for bit), so the kernel equals the float64 mirror."""
    Y, G, rows, X0 = BC.exact_case()
    want = np.stack([BE.block_sweep64(e, Y, G, 1.0, 1.0, X0[r] if warm else None, 16, sweeps) for r, e in enumerate(rows)])
    X, nf = ops.als_block_rows(_csr(rows, Y.shape[0]), _dev(Y), _dev(G), alpha=1.0, reg=1.0, block=16, sweeps=sweeps,
                               x=_dev(X0) if warm else None)
    assert int(nf.item()) == 0 and want.any()
    assert t.equal(X.cpu(), t.from_numpy(want.astype(np.float32)))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


# ---- 3. determinism and row purity ----------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits(case):
    for from_zero, sweeps in ((True, 1), (False, 3)):
        X, _ = case.call(from_zero, sweeps)
        assert t.equal(X, case.out(from_zero, sweeps))


def test_a_row_alone_equals_its_bits_in_the_batch(case):
    """Every row as its own one-row CSR, warm start, three sweeps: the resident and the streaming path alone and in company."""
    want = case.out(False, 3)
    for r in range(N_ROWS):
        X, _ = case.call(False, 3, csr=_csr([case.pr.rows[r]], N_COLS), rows=[r])
        assert t.equal(X[0], want[r]), (case.d, case.B, r)


def test_row_list_in_any_order(case):
    rl = _dev(np.asarray(ROW_LIST, dtype=np.int32))
    for from_zero, sweeps in ((True, 1), (False, 3)):
        X, nf = case.call(from_zero, sweeps, rows=ROW_LIST, row_list=rl)
        assert int(nf.item()) == 0 and X.shape == (len(ROW_LIST), case.d)
        assert t.equal(X, case.out(from_zero, sweeps)[rl.long()])        # compact by list position, the batched call's bits


def test_resident_and_streaming_path_give_the_same_bits():
    """A row one entry longer than the residency constant whose last entry is a zero factor row: the rule gives it the bits of
    the row without that entry (every chain gains fmaf(0, ., acc) == acc), which is resident."""
    d, B = 64, 16
    n = ops.als_block_chunk(d, B)
    rng = np.random.default_rng(3)
    Y = (0.2 + rng.standard_normal((50, d)) * 0.3).astype(np.float32)
    Y[49] = 0.0
    G = BE.sym_lower((Y.T @ Y).astype(np.float32))
    head = rng.integers(0, 49, n).tolist()
    x0 = _dev((rng.standard_normal((1, d)) * 0.1).astype(np.float32)).repeat(2, 1)
    X, nf = ops.als_block_rows(_csr([head, head + [49]], 50), _dev(Y), _dev(G), alpha=ALPHA, reg=REG, block=B, sweeps=2, x=x0)
    assert int(nf.item()) == 0 and X[0].abs().sum() > 0 and t.equal(X[0], X[1])


# ---- 4. failed pivots -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,B", [(16, 16), (40, 16), (128, 32), (256, 64)])
def test_failed_pivots_are_counted_and_zeroed(d, B):
    c = _CASES.setdefault((d, B), Case(d, B))
    before = c.out(False, 3).clone()
    G_bad = _dev(-10.0 * np.eye(d, dtype=np.float32))
    picks = [0, 1, 2, BC.LONG_ROW, 6, 5, 20, 0]                       # two empty rows among them, streaming and resident ones
    rows = [c.pr.rows[r] for r in picks]
    x = t.full((len(rows), d), 0.5, device="cuda")
    X, nf = ops.als_block_rows(_csr(rows, N_COLS), c.Y_dev * 0.01, G_bad, alpha=1.0, reg=0.5, block=B, sweeps=2, x=x)
    assert X is x and int(nf.item()) == sum(1 for r in rows if len(r)) == 6
    assert not X.cpu().numpy().any()
    again, nf2 = c.call(False, 3)
    assert int(nf2.item()) == 0 and t.equal(again, before)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = _CASES.setdefault((16, 16), Case(16, 16))
    kw = dict(alpha=1.0, reg=1.0)
    for d, word in ((6, "multiple of 4"), (260, "4 .. 256")):
        with pytest.raises(ValueError, match=word):
            ops.als_block_rows(c.csr, t.zeros(N_COLS, d, device="cuda"), t.zeros(d, d, device="cuda"), **kw)
    with pytest.raises(ValueError, match="block"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, block=8, **kw)
    with pytest.raises(ValueError, match="sweeps"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, sweeps=0, **kw)
    with pytest.raises(ValueError, match="alpha"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, alpha=-1.0, reg=1.0)
    with pytest.raises(ValueError, match="reg"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, alpha=1.0, reg=0.0)
    with pytest.raises(ValueError, match="G must be"):
        ops.als_block_rows(c.csr, c.Y_dev, t.zeros(8, 8, device="cuda"), **kw)
    with pytest.raises(ValueError, match="one row per column"):
        ops.als_block_rows(c.csr, c.Y_dev[:10], c.G_dev, **kw)
    with pytest.raises(ValueError, match="x must be"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, x=t.zeros(3, 16, device="cuda"), **kw)
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_block_rows(c.csr, c.Y_dev.cpu(), c.G_dev, **kw)
    with pytest.raises(_lib.MiError, match="no CPU fallback"):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, x=t.zeros(N_ROWS, 16), **kw)
    with pytest.raises(TypeError):
        ops.als_block_rows(c.csr, c.Y_dev, c.G_dev, row_list=t.zeros(2, dtype=t.int64, device="cuda"), **kw)
    # the C entry point on real device pointers: by return code, before anything is enqueued
    L = _lib.lib()
    nf = t.zeros(1, dtype=t.int32, device="cuda")
    X = t.full((N_ROWS, 16), 7.0, device="cuda")
    ws = t.empty(L.mi_als_block_rows_workspace_bytes(N_ROWS, c.csr.nnz, 16, 16), dtype=t.uint8, device="cuda")
    misaligned = c.Y_dev.contiguous().reshape(-1)[1:1 + 16 * (N_COLS - 1)].reshape(N_COLS - 1, 16)

    def call(d=16, block=16, sweeps=1, Y=c.Y_dev, ldy=24, n_cols=N_COLS, nnz=c.csr.nnz, alpha=1.0, reg=1.0, ws_bytes=ws.numel()):
        return L.mi_als_block_rows_f32(N_ROWS, d, block, sweeps, c.csr.rowptr.data_ptr(), c.csr.col.data_ptr(), nnz, n_cols,
                                       Y.data_ptr(), ldy, c.G_dev.data_ptr(), alpha, reg, X.data_ptr(), 16, 0, None, 0,
                                       nf.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
    bad = _lib.MI_ERR_BAD_ARG
    assert call(d=6) == bad and call(d=260) == bad and call(d=0) == bad
    assert call(block=8) == bad and call(block=24) == bad and call(sweeps=0) == bad and call(sweeps=65) == bad
    assert call(n_cols=1 << 31) == bad and call(nnz=1 << 31) == bad
    assert call(Y=misaligned, ldy=16) == bad and call(ldy=18) == bad and call(ldy=12) == bad
    assert call(alpha=-1.0) == bad and call(reg=0.0) == bad
    assert call(ws_bytes=ws.numel() - 256) == _lib.MI_ERR_WORKSPACE
    t.cuda.synchronize()
    assert int(nf.item()) == 0 and bool((X == 7.0).all())             # nothing was enqueued


# ---- 6. the trainer -------------------------------------------------------------------------------------------------------------
def _small_graph():
    rng = np.random.default_rng(11)
    pairs = rng.choice(60 * 50, size=500, replace=False)
    return t.from_numpy(np.stack([pairs // 50, pairs % 50]).astype(np.int64))


def test_trainer_at_dim_256_follows_the_float64_half_sweeps():
    """solver="block" at dim 256 on a 60 x 50 graph: after each half-sweep the device objective agrees with the objective after
    a float64 block half-sweep from the same start, within 8 times the relative gap the float32 reference leaves."""
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 50)
    alpha, reg, B = 1.0, 2.0, 16
    model = ImplicitALS(60, 50, dim=256, alpha=alpha, reg=reg, seed=3, solver="block", block=B).cuda()
    ptr_u, idx_u = AE.csr_of(ei[0].numpy(), ei[1].numpy(), 60)
    ptr_i, idx_i = AE.csr_of(ei[1].numpy(), ei[0].numpy(), 50)
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


def test_trainer_fit_fold_in_and_consumers():
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 50)
    kw = dict(dim=256, alpha=1.0, reg=2.0, seed=5, solver="block")
    a = ImplicitALS(60, 50, **kw).cuda().fit(inter, 3)
    b = ImplicitALS(60, 50, **kw).cuda().fit(Interactions(ei.cuda(), 60, 50), 3)
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    assert t.isfinite(a.users_emb.weight).all() and a.users_emb.weight.abs().sum() > 0
    # fold-in of a known user's row: from zero, more sweeps come closer to the user's vector once that vector is the
    # minimiser against the current item table (many warm-started sweeps of the user side)
    a.block_sweeps = 32
    for _ in range(4):
        assert int(a.half_sweep("users").item()) == 0
    csr = inter.csr()
    for u in (0, 17, 59):
        lo, hi = int(csr.rowptr[u]), int(csr.rowptr[u + 1])
        p = t.tensor([0, hi - lo], dtype=t.int32, device="cuda")
        dist = []
        for s in (1, 2, 4, 8):
            a.fold_in_sweeps = s
            dist.append(float((a.fold_in(p, csr.col[lo:hi].contiguous())[0] - a.users_emb.weight[u]).norm()))
        print(f"user {u}: |fold_in - x_u| after 1, 2, 4, 8 sweeps: {dist} (|x_u| {float(a.users_emb.weight[u].norm()):.3e})")
        assert dist[0] > dist[1] > dist[2] > dist[3]
    # the consumers of LightGCN's tables take the module
    users = t.arange(60, dtype=t.int64, device="cuda")
    top = topk_for_users(a.users_emb.weight.detach(), a.items_emb.weight.detach(), users, ei.cuda(), 5)
    assert top.shape == (60, 5)
    seen = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert not any((u, int(i)) in seen for u, row in enumerate(top.cpu().tolist()) for i in row)
    held = t.stack([users[:20], top[:20, 0]])                         # each user's best unseen item as a held-out pair: rank 0
    m = get_full_rank_metrics_lightgcn(a, held, [ei.cuda()], ks=(5,))
    assert m["recall@5"] == 1.0 and abs(m["mrr"] - 1.0) < 1e-12


def test_default_solver_is_the_cholesky_solver_bit_for_bit():
    ei = _small_graph()
    inter = Interactions(ei.cuda(), 60, 50)
    a = ImplicitALS(60, 50, dim=16, alpha=1.0, reg=2.0, seed=5).cuda().fit(inter, 2)
    b = ImplicitALS(60, 50, dim=16, alpha=1.0, reg=2.0, seed=5, solver="cholesky").cuda().fit(inter, 2)
    assert t.equal(a.users_emb.weight, b.users_emb.weight) and t.equal(a.items_emb.weight, b.items_emb.weight)
    c = ImplicitALS(60, 50, dim=16, alpha=1.0, reg=2.0, seed=5, solver="block").cuda().fit(inter, 2)
    assert not t.equal(a.users_emb.weight, c.users_emb.weight)        # the keyword does select another solver


def test_fit_raises_on_failed_rows():
    ei = _small_graph()
    model = ImplicitALS(60, 50, dim=16, alpha=1.0, reg=1.0, seed=0, solver="block").cuda()
    model.items_emb.weight.fill_(float("nan"))                        # every user system has a NaN pivot: arithmetic, no fault
    with pytest.raises(RuntimeError, match="pivot"):
        model.fit(Interactions(ei.cuda(), 60, 50), 1)


# ---- 7. quality -----------------------------------------------------------------------------------------------------------------
def test_planted_graph_beats_popularity():
    """test_gpu_als.py's recipe with the block solver (B = 16, one sweep per half-sweep), d = 64, 5 epochs."""
    spec = S.SyntheticSpec(943, 1682, 100000, seed=5, communities=8, community_mix=0.85, deg_min=1, deg_max=min(2000, 1682 // 2))
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 20000).cuda()
    inter = Interactions(ei.cuda(), spec.num_users, spec.num_items)
    model = ImplicitALS(spec.num_users, spec.num_items, dim=64, alpha=1.0, reg=20.0, seed=0, solver="block").cuda().fit(inter, 5)
    m_als = get_full_rank_metrics_lightgcn(model, held, [inter.edge_index], ks=(12,))["map@12"]
    deg = t.bincount(inter.edge_index[1], minlength=spec.num_items).to(t.float32)
    ue = t.zeros(spec.num_users, 4, device="cuda")
    ue[:, 0] = 1.0
    ie = t.zeros(spec.num_items, 4, device="cuda")
    ie[:, 0] = deg
    m_pop = get_full_rank_metrics_lightgcn(None, held, [inter.edge_index], ks=(12,), embeddings=(ue, ie))["map@12"]
    print(f"map@12: iALS block {m_als:.4f}, popularity {m_pop:.4f}")
    assert m_als > m_pop
