"""The references and bounds of tests/ranker_kernel_refs.py, checked on the CPU: every bound admits a float32 evaluation of the
formula it bounds (it can be met) and refuses a deliberately worse emulation (it is not vacuous); the references agree with
torch's own operators; the test data have the properties the GPU tests rely on."""
import numpy as np
import pytest
import torch as t

import ranker_kernel_refs as K
from oracle import lightgcn_ref as R


# ------------------------------------------------------------------------------------------------------------ batch-norm
@pytest.mark.parametrize("n", K.BN_ROWS)
@pytest.mark.parametrize("c", sorted(set(K.BN_WIDTHS + K.BN_LAYOUT_WIDTHS)))
def test_batchnorm_bounds_admit_float32_and_refuse_float32_sums(n, c):
    x, gamma, beta, dy, rm, rv = K.bn_case(n, c)
    ref = K.bn_fwd_ref(x, gamma, beta, rm, rv)
    bound = K.bn_y_bound(x, ref, gamma)
    assert bool((K.bn_y_worst_case(x, ref, gamma, beta) <= bound).all())       # the issue's bound is a derived one on these data
    hard = t.arange(c) % 4 == 1
    assert bool(((ref["mean"][hard] - 100).abs() < 1).all()) and bool((ref["var"][hard] < 0.1).all())
    y, mu, is_ = K.bn_emulate(x, gamma, beta, double_sums=True)
    sb = K.bn_stat_bounds(n, ref, rm, rv)
    assert bool(((y.double() - ref["y"]).abs() <= bound).all())
    assert bool(((mu.double() - ref["mean"]).abs() <= sb["mean"]).all())
    assert bool(((is_.double() - ref["invstd"]).abs() <= sb["invstd"]).all())
    # torch's own CPU batch-norm against the reference, statistics included
    bn = t.nn.BatchNorm1d(c, eps=K.BN_EPS, momentum=K.BN_MOMENTUM)
    with t.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    yt = bn(x).detach()
    assert bool(((yt.double() - ref["y"]).abs() <= bound).all())
    assert bool(((bn.running_mean.double() - ref["running_mean"]).abs() <= sb["running_mean"]).all())
    assert bool(((bn.running_var.double() - ref["running_var"]).abs() <= sb["running_var"]).all())
    if n > 2:   # two rows: a float32 running sum of two addends is one rounding, there is nothing to get wrong
        bad, _, bad_is = K.bn_emulate(x, gamma, beta, double_sums=False)
        excess = ((bad.double() - ref["y"]).abs() / bound)[:, hard]
        assert float(excess.max()) > 100.0                                      # orders of magnitude, not a near miss
        assert bool(((bad_is.double() - ref["invstd"]).abs() > sb["invstd"])[hard].any())


@pytest.mark.parametrize("n", K.BN_ROWS)
@pytest.mark.parametrize("c", [4, 12, 64, 512])
def test_batchnorm_backward_bounds_admit_float32_and_refuse_a_dropped_row(n, c):
    x, gamma, beta, dy, rm, rv = K.bn_case(n, c)
    _, mu, is_ = K.bn_emulate(x, gamma, beta)
    ref = K.bn_bwd_ref(x, dy, gamma, mu, is_)
    dx, dg, db = K.bn_bwd_emulate(x, dy, gamma, mu, is_)
    for got, key in ((dx, "dx"), (dg, "dgamma"), (db, "dbeta")):
        assert bool(((got.double() - ref[key]).abs() <= ref[key + "_bound"]).all()), key
    # autograd through torch's batch-norm agrees with the float64 formulas (double: far inside any float32 bound)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    (t.nn.functional.batch_norm(xd, None, None, gd, bd, True, 0.0, K.BN_EPS) * dy.double()).sum().backward()
    ref_d = K.bn_bwd_ref(x, dy, gamma, K.bn_fwd_ref(x, gamma, beta, rm, rv)["mean"], K.bn_fwd_ref(x, gamma, beta, rm, rv)["invstd"])
    scale = float(xd.grad.abs().max()) + 1e-30
    assert float((xd.grad - ref_d["dx"]).abs().max()) <= 1e-9 * scale
    assert t.allclose(gd.grad, ref_d["dgamma"], rtol=1e-9, atol=1e-9) and t.allclose(bd.grad, ref_d["dbeta"], rtol=1e-9, atol=1e-9)
    # worse: the sums miss the last row
    dx2, dg2, db2 = K.bn_bwd_emulate(x[:-1], dy[:-1], gamma, mu, is_)
    assert bool(((dg2.double() - ref["dgamma"]).abs() > ref["dgamma_bound"]).any())
    assert bool(((db2.double() - ref["dbeta"]).abs() > ref["dbeta_bound"]).any())


# ------------------------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("n", K.BCE_SIZES)
def test_bce_bounds_admit_float32_with_a_double_sum_and_refuse_a_float32_running_sum(n):
    x, y = K.bce_case(n)
    assert bool(t.isfinite(x).all()) and bool(((y >= 0) & (y <= 1)).all())
    if n > 1:
        assert int(((y > 0) & (y < 1)).sum()) >= 5 and set(t.tensor(K.BCE_PLANTS).tolist()) <= set(x.tolist())
    ref = K.bce_ref(x, y)
    want = t.nn.functional.binary_cross_entropy_with_logits(x.double(), y.double())
    assert abs(float(ref["loss"] - want)) <= 1e-12 * float(want)
    loss, dx = K.bce_emulate(x, y)
    assert abs(loss - float(ref["loss"])) <= float(ref["loss_bound"])
    assert float((dx.double() - ref["dx"]).abs().max()) <= ref["dx_bound"]
    if n == 5000:
        # a float32 running sum is a random walk of ~5000 roundings at the size of the partial sum: one draw in a few ends near
        # the exact value by luck, so six draws are taken — the double sum passes all, the running sum fails most
        missed = 0
        for seed in range(6):
            xs, ys = K.bce_case(n, seed)
            rs = K.bce_ref(xs, ys)
            assert abs(K.bce_emulate(xs, ys)[0] - float(rs["loss"])) <= float(rs["loss_bound"])
            missed += abs(K.bce_emulate(xs, ys, float_sum=True)[0] - float(rs["loss"])) > float(rs["loss_bound"])
        assert missed >= 4


# ---------------------------------------------------------------------------------------------------------- embed_concat
@pytest.mark.parametrize("name", [c[0] for c in K.EMBED_CASES])
def test_embed_bound_admits_float32_and_refuses_a_bfloat16_norm(name):
    tables, x = K.embed_case(name)
    want, bound, near = K.embed_ref(x, tables, 1.0)
    assert near == 0
    torch_want = t.cat([t.nn.functional.embedding(x[:, i], tb.double().clone(), max_norm=1.0) for i, tb in enumerate(tables)], 1)
    assert t.allclose(want, torch_want, rtol=1e-12, atol=0)
    got = K.embed_emulate(x, tables, 1.0)
    assert bool(((got.double() - want).abs() <= bound).all())
    norms = t.cat([tb[x[:, i]].double().norm(dim=1) for i, tb in enumerate(tables)])
    if bool((norms > 1).any()):
        bad = K.embed_emulate(x, tables, 1.0, bad_norm=True)
        assert bool(((bad.double() - want).abs() > bound).any())
    if name == "twenty":   # both branches inside one call, and inside its second group of columns
        assert bool((norms > 1).any()) and bool((norms < 1).any())
    plain, _, _ = K.embed_ref(x, tables, 0.0)
    assert t.equal(plain, t.cat([tb.double()[x[:, i]] for i, tb in enumerate(tables)], 1))


# ------------------------------------------------------------------------------------------------------------ segment max
def _segmax_loop(src, dst, X, n_dst):
    """The kernel's loop: sources of a destination in sorted order, `who < 0 or v > best`."""
    d = X.shape[1]
    Y, arg = np.zeros((n_dst, d), np.float32), np.full((n_dst, d), -1, np.int64)
    Xn = X.numpy()
    for r in range(n_dst):
        for s in sorted(set(src[dst == r].tolist())):
            take = (arg[r] < 0) | (Xn[s] > Y[r])
            Y[r] = np.where(take, Xn[s], Y[r])
            arg[r] = np.where(take, s, arg[r])
    return t.from_numpy(Y), t.from_numpy(arg)


@pytest.mark.parametrize("n_dst", K.SEG_DSTS)
@pytest.mark.parametrize("d", [1, 65])
def test_segment_max_reference_is_the_documented_rule_and_its_data_hold_the_edges(n_dst, d):
    src, dst, X, dY = K.segmax_case(n_dst, d)
    Y, arg = K.segmax_ref(src, dst, X, n_dst)
    Yl, argl = _segmax_loop(src, dst, X, n_dst)
    assert t.equal(Y, Yl.double()) and t.equal(arg, argl)
    assert not bool(((arg == 7) | (arg == 9)).any()) and bool((arg == 2).any())           # ties: the smallest id
    assert len(set(zip(src.tolist(), dst.tolist()))) < src.numel()                           # duplicated edges
    if n_dst > 1:
        assert bool((arg[0] == -1).all()) and bool((arg[-1] == -1).all()) and bool((Y[0] == 0).all()) and bool((Y[-1] == 0).all())
        assert bool(((Y == float("-inf")) & (arg == 11)).any())                              # all -inf: first source
        assert bool(((Y < -1) & (arg >= 13) & (arg <= 14)).any())                            # all negative: not the empty 0
    ref, bound = K.segmax_bwd_ref(arg, dY, K.SEG_SRC)
    seq = np.zeros((K.SEG_SRC, d), np.float32)
    for r in range(n_dst):                                                                   # float32, destination order
        for c in range(d):
            if arg[r, c] >= 0:
                seq[arg[r, c], c] += dY[r, c].item()
    assert bool(((t.from_numpy(seq).double() - ref).abs() <= bound).all())
    assert bool((ref[7] == 0).all()) and bool((ref[9] == 0).all())
    if n_dst == 203:
        half = np.zeros((K.SEG_SRC, d), np.float16)                                          # worse: a float16 accumulator
        for r in range(n_dst):
            for c in range(d):
                if arg[r, c] >= 0:
                    half[arg[r, c], c] += np.float16(dY[r, c].item())
        assert bool(((t.from_numpy(half.astype(np.float64)) - ref).abs() > bound).any())


# ------------------------------------------------------------------------------------------------------------ CSR builders
@pytest.mark.parametrize("n_rows,n_cols", K.CSR_SHAPES)
def test_coo_cases_hold_what_the_gpu_tests_need(n_rows, n_cols):
    for variant in ("largest", "empty_ends"):
        if variant == "empty_ends" and n_rows < 3:
            continue
        row, col = K.coo_case(n_rows, n_cols, variant)
        assert int(row.min()) >= 0 and int(row.max()) < n_rows and int(col.min()) >= 0 and int(col.max()) < n_cols
        key = row * n_cols + col
        assert key.unique().numel() < key.numel()                                            # duplicates
        rowptr, col_s, perm = R.sparse_tensor_csr(row, col, n_rows, n_cols)
        if variant == "largest":
            assert int(key.max()) == n_rows * n_cols - 1 and int(col[row == 0].max()) == n_cols - 1
        else:
            assert int(rowptr[1]) == 0 and int(rowptr[-2]) == int(rowptr[-1])
        # an unstable sort shows: some run of equal keys is out of input order under a reversed tie-break
        rev = t.argsort(key.flip(0), stable=True)
        assert not t.equal(row.numel() - 1 - rev, perm)


@pytest.mark.parametrize("d", K.SEG_WIDTHS)
@pytest.mark.parametrize("n_dst", K.SEG_DSTS)
def test_segment_max_data_put_the_tied_source_on_top_at_every_shape(n_dst, d):
    src, dst, X, _ = K.segmax_case(n_dst, d)
    assert t.equal(X[7], X[2]) and t.equal(X[9], X[2]) and int(dst.max()) < n_dst and int(src.max()) < K.SEG_SRC
    _, arg = K.segmax_ref(src, dst, X, n_dst)
    with27 = t.tensor([{2, 7, 9} <= set(src[dst == r].tolist()) for r in range(n_dst)])
    assert bool(with27.any()) and bool((arg[with27] == 2).any()) and not bool(((arg == 7) | (arg == 9)).any())
    assert not bool(((src == 7) | (src == 9))[~with27[dst]].any())                           # 7 and 9 never without 2


# ------------------------------------------------------------------------------------ batch_norm() beyond the kernels' width
@pytest.mark.parametrize("momentum", [0.1, None])
def test_batch_norm_wrapper_beyond_512_channels_is_torch_batchnorm1d(momentum):
    """The module wrapper hands layers wider than the kernels' 512 channels to torch's batch_norm: on the CPU that is the very
    operator BatchNorm1d runs, so outputs, gradients and every buffer are equal, not close."""
    from laplace_amd import ops
    from laplace_amd.model.encoder_decoder import batch_norm
    c = ops.BATCHNORM_MAX_CHANNELS + 8
    g = t.Generator().manual_seed(c)
    x, w = t.randn(40, c, generator=g) * 2 + 1, t.randn(40, c, generator=g)
    ref = t.nn.BatchNorm1d(c, momentum=momentum)
    with t.no_grad():
        ref.weight.copy_(t.rand(c, generator=g) + 0.5)
        ref.bias.copy_(t.randn(c, generator=g))
    mine = t.nn.BatchNorm1d(c, momentum=momentum)
    mine.load_state_dict(ref.state_dict())
    for it in range(3):
        xr, xm = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        yr, ym = ref(xr), batch_norm(mine, xm)
        assert t.equal(yr, ym)
        ref.zero_grad(); mine.zero_grad()
        (yr * w).sum().backward(); (ym * w).sum().backward()
        assert t.equal(xr.grad, xm.grad) and t.equal(ref.weight.grad, mine.weight.grad) and t.equal(ref.bias.grad, mine.bias.grad)
        for k, v in ref.state_dict().items():
            assert t.equal(v, mine.state_dict()[k]), k
        assert int(mine.num_batches_tracked) == it + 1
    ref.eval(); mine.eval()
    assert t.equal(ref(x), batch_norm(mine, x)) and int(mine.num_batches_tracked) == 3
