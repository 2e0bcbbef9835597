"""bf16 layer tables on the GPU (csrc/spmm_bf16.hip; the rule is in include/laplace_hip.h): the conversion pass bit for bit, the
product against float64 inside the derived bounds of tests/bf16_layers_emulation.py at every plan x width x form, an exact
case, the bit equalities the rule promises, the argument errors, and the trainer's two step forms.

Not asserted: a bound on |table_bf16 - table_f32| after one step.  Adam's first update is lr * g / (|g| + eps): it is not
Lipschitz in the gradient (a gradient element near zero may change sign), so the bound that follows from
|final_bf16 - final_f32| <= (K - 1) u16 max|layer| is the trivial 2 lr; README says so."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch as t

import bf16_layers_emulation as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
_REF = {}


def _ops():
    from laplace_amd import ops
    return ops


def _bits(x):
    return x.view(t.int16 if x.dtype is t.bfloat16 else t.int32)


class _Graph:
    def __init__(self, rowptr, col, val):
        self.np = (rowptr, col, val)
        self.dev = tuple(t.from_numpy(x).to(DEV) for x in (rowptr, col, val))
        self.plans = {}

    def csr(self):
        """A fresh container on the same device arrays: no test sees a plan another one built."""
        return _ops().DeviceCSR(E.N_ROWS, E.N_COLS, *self.dev)

    def plan(self, key):
        if key is not None and key not in self.plans:
            self.plans[key] = _ops().build_spmm_plan(self.csr(), chunk=key[0], band=key[1])
        return self.plans.get(key)


@pytest.fixture(scope="module")
def graph():
    return _Graph(*E.adjacency())


@pytest.fixture(scope="module")
def exact_graph():
    rowptr, col, val, _ = E.exact_case(8)
    return _Graph(rowptr, col, val)


def _reference(graph, d):
    """float64 reference of the width, computed once and left unchanged."""
    if d not in _REF:
        x, addend = E.operand(d)
        _REF[d] = (x, addend) + E.spmm_f64(*graph.np, x)
    return _REF[d]


def _padded(n, d, dtype, pad, fill=None):
    buf = t.empty(n, d + pad, dtype=dtype, device=DEV)
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :d]


def _run(graph, plan_key, x, *, want_y=False, want_s=False, addend=None, scale=1.0, rows=None, n_dev=None, pad=0, fill=None):
    """ops.spmm_bf16 with an explicit plan (None = the adjacency's own rule: no plan at this size without a row list)."""
    ops = _ops()
    d = x.shape[1]
    X = _padded(E.N_COLS, d, t.bfloat16, pad)
    X.copy_(E.bf16_tensor(x))
    n_out = E.N_ROWS if rows is None else len(rows)
    Y = _padded(n_out, d, t.bfloat16, pad, fill) if want_y else None
    S = _padded(n_out, d, t.float32, pad, fill) if want_s else None
    A = None
    if addend is not None:
        A = _padded(n_out, d, t.float32, pad)
        A.copy_(t.from_numpy(np.ascontiguousarray(addend)))
    kw = {}
    if rows is not None:
        kw = dict(row_list=t.from_numpy(rows).to(DEV),
                  n_list_dev=None if n_dev is None else t.tensor([n_dev], dtype=t.int32, device=DEV))
    if rows is not None and plan_key is None:
        # ops.spmm_bf16 gives a row list the adjacency's default plan; the plan-less listed launch is reached through the C ABI
        from laplace_amd import _lib
        ptr = lambda z: None if z is None else z.data_ptr()
        ld = lambda z: 0 if z is None else z.stride(0)
        rowptr, col, val = graph.dev
        rc = _lib.lib().mi_spmm_csr_bf16(E.N_ROWS, d, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), X.data_ptr(), ld(X),
                                         ptr(Y), ld(Y), ptr(A), ld(A), ptr(S), ld(S), float(scale), None,
                                         kw["row_list"].data_ptr(), ptr(kw["n_list_dev"]), len(rows), 0, None, 0,
                                         t.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        ops.spmm_bf16(graph.csr(), X, Y=Y, addend=A, S=S, scale=scale, plan=graph.plan(plan_key), **kw)
    t.cuda.synchronize()
    return Y, S


def _f64(x):
    return x.float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------- the conversion
def test_rows_to_bf16_is_round_to_nearest_even_bit_for_bit():
    ops = _ops()
    special = np.array([0x3F808000, 0xBF808000,      # ties, kept mantissa even: down to 0x3F80
                        0x3F818000, 0xBF818000,      # ties, kept mantissa odd: up to 0x3F82
                        0x3F807FFF, 0x3F808001, 0xBF807FFF, 0xBF808001,   # either side of a tie
                        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,   # +-0, +-inf
                        0x7F7FFFFF, 0xFF7FFFFF,      # the largest finite f32 rounds to inf
                        0x7F7F7FFF, 0x7F7F8000,      # the largest bf16 from below; the tie above it goes to inf (odd mantissa)
                        0x3F7FFFFF, 0x477FE000], dtype=np.uint32).view(F)
    rng = np.random.default_rng(11)
    table = (rng.standard_normal((37, 24)) * np.exp2(rng.integers(-20, 20, size=(37, 24)))).astype(F)
    table.reshape(-1)[: special.size] = special
    src = t.from_numpy(table).to(DEV)
    want = t.from_numpy(table).to(t.bfloat16)
    got = ops.rows_to_bf16(src)
    assert got.dtype is t.bfloat16 and t.equal(_bits(got.cpu()), _bits(want))
    w = _bits(want).reshape(-1)[: special.size].numpy().view(np.uint16)
    assert list(w[:4]) == [0x3F80, 0xBF80, 0x3F82, 0xBF82] and list(w[8:14]) == [0, 0x8000, 0x7F80, 0xFF80, 0x7F80, 0xFF80]
    # strided source and destination, out=
    wide = t.zeros(37, 32, device=DEV)
    wide[:, :24] = src
    out = _padded(37, 24, t.bfloat16, 8, fill=7.0)
    assert ops.rows_to_bf16(wide[:, :24], out=out) is out
    assert t.equal(_bits(out.cpu().contiguous()), _bits(want))
    assert bool((out.as_strided((37, 8), (32, 1), 24) == 7.0).all())          # the padding is not written


# ----------------------------------------------------------------------------------------------- the product vs float64
@pytest.mark.parametrize("plan_key", E.PLANS)
@pytest.mark.parametrize("d,pad", [(8, 0), (24, 0), (64, 0), (128, 0), (256, 0), (24, 8)])
def test_spmm_bf16_within_the_derived_bounds(graph, plan_key, d, pad):
    x, addend, exact, absum, n = _reference(graph, d)
    add64 = addend.astype(np.float64)
    # Y alone
    Y, _ = _run(graph, plan_key, x, want_y=True, pad=pad)
    assert (np.abs(_f64(Y) - exact) <= E.bound_y(n, absum, exact)).all()
    # S alone: the unrounded sum
    _, S = _run(graph, plan_key, x, want_s=True, addend=addend, scale=0.25, pad=pad)
    assert (np.abs(_f64(S) - 0.25 * (add64 + exact)) <= E.bound_s(n, absum, exact, addend, 0.25)).all()
    # both: S takes the rounded layer
    Y2, S2 = _run(graph, plan_key, x, want_y=True, want_s=True, addend=addend, scale=-2.0, pad=pad)
    assert t.equal(_bits(Y2.contiguous()), _bits(Y.contiguous()))
    assert (np.abs(_f64(S2) - (-2.0) * (add64 + exact)) <= E.bound_s_with_y(n, absum, exact, addend, -2.0)).all()
    want_s2 = (t.from_numpy(addend).to(DEV) + Y2.float()) * -2.0
    assert t.equal(S2, want_s2)                                       # S = scale * (addend + float(rn(acc))), one rounding each
    # row list (compact addend and outputs)
    rows, _ = E.row_list()
    Yl, Sl = _run(graph, plan_key, x, want_y=True, want_s=True, addend=addend[rows], scale=0.5, rows=rows, pad=pad)
    assert (np.abs(_f64(Yl) - exact[rows]) <= E.bound_y(n[rows], absum[rows], exact[rows])).all()
    assert (np.abs(_f64(Sl) - 0.5 * (add64[rows] + exact[rows]))
            <= E.bound_s_with_y(n[rows], absum[rows], exact[rows], addend[rows], 0.5)).all()


@pytest.mark.parametrize("plan_key", E.PLANS)
@pytest.mark.parametrize("d", [8, 24, 128, 256])
def test_exact_case_equals_the_integer_reference(exact_graph, plan_key, d):
    """Every f32 sum is exact, so a wrong index, a dropped entry or a lost partial row shows outright."""
    rowptr, col, val, x = E.exact_case(d)
    exact, _, _ = E.spmm_f64(rowptr, col, val, x)
    want = t.from_numpy(exact)
    _, S = _run(exact_graph, plan_key, x, want_s=True)
    assert t.equal(S.cpu().double(), want)
    Y, _ = _run(exact_graph, plan_key, x, want_y=True)
    assert t.equal(_bits(Y.cpu().contiguous()), _bits(want.float().to(t.bfloat16)))
    rows, n_dev = E.row_list()
    _, Sl = _run(exact_graph, plan_key, x, want_s=True, rows=rows, n_dev=n_dev, fill=-7.0)
    assert t.equal(Sl[:n_dev].cpu().double(), want[rows[:n_dev]]) and bool((Sl[n_dev:] == -7.0).all())


# ------------------------------------------------------------------------------------------------------- bit equalities
@pytest.mark.parametrize("plan_key", E.PLANS)
@pytest.mark.parametrize("d", [24, 128])
def test_bit_equalities(graph, plan_key, d, monkeypatch):
    ops = _ops()
    x, addend, *_ = _reference(graph, d)
    kw = dict(want_y=True, want_s=True, addend=addend, scale=0.25)
    monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", 1)
    Y1, S1 = _run(graph, plan_key, x, **kw)
    Y2, S2 = _run(graph, plan_key, x, **kw)
    assert t.equal(_bits(Y1), _bits(Y2)) and t.equal(_bits(S1), _bits(S2))                 # run to run
    monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", 0)
    Y0, S0 = _run(graph, plan_key, x, **kw)
    assert t.equal(_bits(Y1), _bits(Y0)) and t.equal(_bits(S1), _bits(S0))                 # one stream or two
    _, U1 = _run(graph, plan_key, x, want_s=True, addend=addend, scale=0.25)               # the unrounded sum, for the list below
    for streams in (0, 1):
        monkeypatch.setattr(ops, "SPMM_TWO_STREAMS", streams)
        rows, n_dev = E.row_list()
        Yl, Sl = _run(graph, plan_key, x, rows=rows, n_dev=n_dev, fill=3.0, **dict(kw, addend=addend[rows]))
        idx = t.from_numpy(rows[:n_dev]).long().to(DEV)
        assert t.equal(_bits(Yl[:n_dev]), _bits(Y1[idx])) and t.equal(_bits(Sl[:n_dev]), _bits(S1[idx]))   # listed = dense
        assert bool((Yl[n_dev:] == 3.0).all()) and bool((Sl[n_dev:] == 3.0).all())         # beyond the device count: untouched
        _, Ul = _run(graph, plan_key, x, want_s=True, addend=addend[rows], scale=0.25, rows=rows)
        assert t.equal(_bits(Ul), _bits(U1[t.from_numpy(rows).long().to(DEV)]))


def test_gather_rows_from_a_bf16_table():
    ops = _ops()
    g = t.Generator().manual_seed(2)
    src = t.randn(50, 24, generator=g).to(t.bfloat16).to(DEV)
    rows = t.tensor([3, 49, 0, 3, 17, 20, 9], dtype=t.int32, device=DEV)
    cnt = t.tensor([5], dtype=t.int32, device=DEV)
    base = t.randn(7, 24, generator=g).to(DEV)
    dst = base.clone()
    ops.gather_rows(dst, src, rows, cnt, accumulate=True)
    assert t.equal(dst[:5], base[:5] + src[rows[:5].long()].float()) and t.equal(dst[5:], base[5:])
    dst = base.clone()
    ops.gather_rows(dst, src, rows, cnt)
    assert t.equal(dst[:5], src[rows[:5].long()].float()) and t.equal(dst[5:], base[5:])
    wide = t.full((7, 32), 9.0, device=DEV)
    ops.gather_rows(wide[:, :24], src, rows)                                                # no device count, strided dst
    assert t.equal(wide[:, :24], src[rows.long()].float()) and bool((wide[:, 24:] == 9.0).all())
    with pytest.raises(ValueError, match="bf16"):
        ops.gather_rows(dst, src, rows, scale=0.5)


# ------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_their_code_and_write_nothing(graph):
    from laplace_amd import _lib
    L = _lib.lib()
    rowptr, col, val = graph.dev
    plan = graph.plan((8, 0))
    d = 24
    X = t.zeros(E.N_COLS + 1, 32, dtype=t.bfloat16, device=DEV)
    Y = t.full((E.N_ROWS, 32), 5.0, dtype=t.bfloat16, device=DEV)
    S = t.full((E.N_ROWS, 32), 5.0, device=DEV)
    ws = t.empty(int(L.mi_spmm_workspace_bytes(ctypes.byref(plan.struct), d)), dtype=t.uint8, device=DEV)
    stream = t.cuda.current_stream().cuda_stream

    def call(d=d, x=X.data_ptr(), ldx=32, y=Y.data_ptr(), ldy=32, s=S.data_ptr(), lds=32, parts=0, plan=plan,
             ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), rows=None, n_list=0):
        return L.mi_spmm_csr_bf16(E.N_ROWS, d, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), x, ldx, y, ldy, None, 0, s, lds,
                                  1.0, ctypes.byref(plan.struct) if plan is not None else None, rows, None, n_list, parts,
                                  ws_ptr, ws_bytes, stream)
    bad, unsupported, workspace = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_UNSUPPORTED, _lib.MI_ERR_WORKSPACE
    assert call(d=20) == bad and call(d=0) == bad                    # widths
    assert call(d=264, ldx=264, ldy=264, lds=264) == unsupported
    assert call(x=X.data_ptr() + 2) == bad and call(y=Y.data_ptr() + 8) == bad and call(s=S.data_ptr() + 4) == bad   # alignment
    assert call(ldx=28) == bad and call(ldy=20) == bad and call(lds=22) == bad and call(ldx=16) == bad   # leading dimensions
    assert call(y=X.data_ptr()) == bad and call(s=X.data_ptr()) == bad                     # aliasing
    assert call(y=None, s=None) == bad and call(parts=4) == bad and call(n_list=3) == bad
    assert call(ws_ptr=None) == workspace and call(ws_bytes=ws.numel() - 512) == workspace
    assert L.mi_rows_f32_to_bf16(4, 12, S.data_ptr(), 32, Y.data_ptr(), 32, stream) == bad
    assert L.mi_rows_f32_to_bf16(4, 24, S.data_ptr(), 32, Y.data_ptr(), 28, stream) == bad
    assert L.mi_rows_f32_to_bf16(4, 24, S.data_ptr() + 4, 32, Y.data_ptr(), 32, stream) == bad
    assert L.mi_gather_rows_bf16_f32(4, None, 24, rowptr.data_ptr(), X.data_ptr(), 28, S.data_ptr(), 32, 0, stream) == bad
    assert L.mi_gather_rows_bf16_f32(4, None, 20, rowptr.data_ptr(), X.data_ptr(), 32, S.data_ptr(), 32, 0, stream) == bad
    t.cuda.synchronize()
    assert bool((Y == 5.0).all()) and bool((S == 5.0).all()) and bool((X == 0).all())
    assert call() == 0                                                # and the same call with nothing wrong runs
    t.cuda.synchronize()
    assert bool((S[:, :d] == 0).all()) and bool((S[:, d:] == 5.0).all())
    # ops: the checks a caller meets first
    ops = _ops()
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.spmm_bf16(graph.csr(), t.zeros(E.N_COLS, 12, dtype=t.bfloat16, device=DEV), S=t.zeros(E.N_ROWS, 12, device=DEV))
    with pytest.raises(TypeError):
        ops.spmm_bf16(graph.csr(), t.zeros(E.N_COLS, 16, device=DEV), S=t.zeros(E.N_ROWS, 16, device=DEV))


def test_default_plan_slot_leaves_the_f32_plan_alone(graph):
    """A row list builds a.plan_bf16 (work items only) and never touches a.plan; an explicit plan= overrides it."""
    ops = _ops()
    a = graph.csr()
    x, *_ = _reference(graph, 24)
    X = E.bf16_tensor(x).to(DEV)
    rows, _ = E.row_list()
    S = t.empty(len(rows), 24, device=DEV)
    ops.spmm_bf16(a, X, S=S, row_list=t.from_numpy(rows).to(DEV))
    assert a.plan is None and a.plan_bf16 is not None and a.plan_bf16.sweep is None and a.plan_bf16.n_thin_rows == 0
    assert int(a.plan_bf16.struct.chunk) == ops.DEFAULT_CHUNK and a.plan_bf16.n_split_rows == 1    # the 257-entry row
    S8 = t.empty_like(S)
    ops.spmm_bf16(a, X, S=S8, row_list=t.from_numpy(rows).to(DEV), plan=graph.plan((8, 64)))
    exact, absum, n = _reference(graph, 24)[2:]
    for got in (S, S8):
        assert (np.abs(_f64(got) - exact[rows]) <= E.bound_s(n[rows], absum[rows], exact[rows], None, 1.0)).all()


# -------------------------------------------------------------------------------------------------------------- trainer
U, I, EDGES, D, B = 300, 200, 3000, 16, 256


def _trainer(K=3, reorder=False, **kw):
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    g = t.Generator().manual_seed(5)
    ei = t.stack([t.randint(0, U, (EDGES,), generator=g), t.randint(0, I, (EDGES,), generator=g)])
    t.manual_seed(5)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K).to(DEV)
    inter = Interactions(ei, U, I)
    adj = inter.adjacency("bipartite")
    kw.setdefault("lr", 1e-3)
    return LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), Lambda=1e-4, batch_size=B, seed=9, reorder=reorder, **kw)


@pytest.mark.parametrize("reorder", [False, True])
def test_dense_forward_is_the_rule_run_op_by_op(reorder):
    ops = _ops()
    K = 3
    tr = _trainer(K, reorder, layer_dtype="bf16", sparse_batch=False)
    final = tr.forward(layer_dtype="bf16").clone()
    tab, adj = tr.table, tr.adj_fwd
    x = ops.rows_to_bf16(tab)
    assert t.equal(_bits(x), _bits(tab.to(t.bfloat16)))
    run = tab.clone()
    for _ in range(1, K):
        y = t.empty_like(x)
        ops.spmm_bf16(adj, x, Y=y)
        run = run + y.float()
        x = y
    acc = t.empty_like(tab)
    ops.spmm_bf16(adj, x, S=acc)
    assert t.equal(final, (run + acc) * (1.0 / (K + 1)))
    # the trainer's forward() stays the f32 one: evaluation and serving do not change
    f32 = _trainer(K, reorder, sparse_batch=False)
    assert t.equal(tr.forward(), f32.forward()) and not t.equal(tr.forward(), final)


@pytest.mark.parametrize("K,reorder", [(1, False), (2, False), (3, False), (3, True), (4, True)])
def test_sparse_batch_step_trains_on_the_dense_forward(K, reorder):
    """final_c equals the dense bf16 forward at the batch's nodes bit for bit, and one step of each form gives the same table
    within the tolerance the f32 forms are held to (tests/test_gpu_lightgcn.py, sparse against plain: 2e-6)."""
    dense = _trainer(K, reorder, layer_dtype="bf16", sparse_batch=False)
    fast = _trainer(K, reorder, layer_dtype="bf16", sparse_batch=True)
    assert len(fast.x_bf16) == min(K, 3) and all(x.dtype is t.bfloat16 for x in fast.x_bf16)
    final = dense.forward(layer_dtype="bf16").clone()
    la, lb = float(dense.step()), float(fast.step())
    assert t.equal(dense.batch_idx[0], fast.batch_idx[0]) and t.equal(dense.batch_idx[2], fast.batch_idx[2])
    cnt = int(fast.n_nodes[0])
    assert cnt > B
    assert t.equal(fast.final_c[:cnt], final[fast.nodes[:cnt].long()])
    assert abs(la - lb) <= 1e-6
    assert (dense.table - fast.table).abs().max() <= 2e-6


@pytest.mark.parametrize("kw", [dict(), dict(sparse_batch=False), dict(objective="bpr", n_neg=4),
                                dict(objective="softmax", n_neg=4, negatives="popularity"),
                                dict(objective="softmax", negatives="in_batch", in_batch_group=64),
                                dict(objective="softmax", full_softmax=True, sparse_batch=False)],
                         ids=["sparse", "dense", "bpr4", "softmax-pop", "in-batch", "full-softmax"])
def test_ten_steps_lower_the_loss(kw):
    tr = _trainer(3, layer_dtype="bf16", lr=1e-2, **kw)
    batch = tr.sample()
    losses = [float(tr.step(batch)) for _ in range(10)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_k0_stores_no_layer_and_steps():
    tr = _trainer(0, layer_dtype="bf16")
    assert tr.x_bf16 == ()
    ref = _trainer(0)
    tr.step(), ref.step()
    assert t.equal(tr.table, ref.table)


@pytest.mark.parametrize("reorder,want", [(False, "75573024e9bf846a"), (True, "30ca95c6e2c4c550")])
@pytest.mark.parametrize("sparse_batch", [True, False])
def test_default_trainer_is_bit_identical_to_the_parent(reorder, want, sparse_batch):
    """The default (layer_dtype="f32") launches what it launched before the bf16 option existed.  Recorded from a run of the
    parent commit on an MI355X, this file's _trainer(3, reorder, sparse_batch=...), three steps, sha256 of the table's bytes,
    first 16 hex digits: reorder off 75573024e9bf846a, reorder on 30ca95c6e2c4c550 (both step forms give the same bits at this
    size)."""
    tr = _trainer(3, reorder, sparse_batch=sparse_batch)
    assert tr.layer_dtype == "f32" and tr.x_bf16 == ()
    for _ in range(3):
        tr.step()
    t.cuda.synchronize()
    assert hashlib.sha256(tr.table.cpu().numpy().tobytes()).hexdigest()[:16] == want
