"""The ranker's element kernels and CSR builders, each called directly through ops and compared with the float64 references and
derived bounds of tests/ranker_kernel_refs.py (csrc/norm.hip: batch-norm, BCE, gather_cat; csrc/sage.hip: segment max,
embed_concat; csrc/csr.hip: COO -> CSR, transpose, scale_csr, expand_rows) — at the widths, row counts and layouts where their
dispatchers change path.  Integer work and copies are compared exactly."""
import pytest
import torch as t

import ranker_kernel_refs as K
from oracle import lightgcn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from laplace_amd import ops
    return ops


def _within(got, want, bound):
    """Largest |got - want| / bound over the elements (0 / 0 counts as 0): <= 1 passes."""
    err = (got.detach().cpu().double() - want).abs()
    ratio = t.where(err == 0, t.zeros_like(err), err / t.as_tensor(bound, dtype=t.float64).expand_as(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def _layout(x, how):
    """x [n, c] on the GPU in the named layout (K.BN_LAYOUTS): the same values behind another leading dimension / base."""
    n, c = x.shape
    if how == "contiguous":
        return x.to(DEV)
    if how in ("ld+4", "ld+1", "ld+3"):
        buf = t.full((n, c + int(how[3:])), float("nan"), device=DEV)
        v = buf[:, :c]
        v.copy_(x)
        assert v.stride() == (c + int(how[3:]), 1) or c <= 1 or n <= 1
        return v
    assert how == "offset1"
    flat = t.full((n * c + 1,), float("nan"), device=DEV)
    v = flat[1:].view(n, c)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------------ batch-norm
def _bn_run(x, gamma, beta, dy, rm, rv, lay_x, lay_dy):
    ops = _ops()
    rm_g, rv_g = rm.to(DEV), rv.to(DEV)
    xg = _layout(x, lay_x)
    y, sm, si = ops.batchnorm_fwd(xg, gamma.to(DEV), beta.to(DEV), rm_g, rv_g, K.BN_MOMENTUM, K.BN_EPS, True)
    dx, dg, db = ops.batchnorm_bwd(xg, _layout(dy, lay_dy), gamma.to(DEV), sm, si)
    return dict(y=y, mean=sm, invstd=si, running_mean=rm_g, running_var=rv_g, dx=dx, dgamma=dg, dbeta=db)


def _bn_check(n, c, lay_x, lay_dy):
    x, gamma, beta, dy, rm, rv = K.bn_case(n, c)
    ref = K.bn_fwd_ref(x, gamma, beta, rm, rv)
    got = _bn_run(x, gamma, beta, dy, rm, rv, lay_x, lay_dy)
    bounds = K.bn_stat_bounds(n, ref, rm, rv)
    bounds["y"] = K.bn_y_bound(x, ref, gamma)
    worst = {k: _within(got[k], ref[k], bounds[k]) for k in ("y", "mean", "invstd", "running_mean", "running_var")}
    bref = K.bn_bwd_ref(x, dy, gamma, got["mean"].cpu(), got["invstd"].cpu())        # from the statistics the forward saved
    for k in ("dx", "dgamma", "dbeta"):
        worst[k] = _within(got[k], bref[k], bref[k + "_bound"])
        bounds[k] = bref[k + "_bound"]
    print(f"batchnorm n={n} c={c} x:{lay_x} dy:{lay_dy} error/bound: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    again = _bn_run(x, gamma, beta, dy, rm, rv, lay_x, lay_dy)
    for k in got:
        assert t.equal(got[k], again[k]), k                                          # fixed reduction order: the same bits
    return got, bounds


@pytest.mark.parametrize("n", K.BN_ROWS)
@pytest.mark.parametrize("c", K.BN_WIDTHS)
def test_batchnorm_every_width_class_against_float64(n, c):
    """c = 4 .. 256 powers of two: the 16-byte partial walk, lpr = c / 4 from 1 (six xor steps) to 64 (none); 12 and 68: scalar
    walk with the vec4 apply; 512: the last supported width (one thread per channel in bn_sum_parts).  Every fourth column has
    mean ~100 and spread 0.1: float32 sums of x^2 miss the bound for y by orders of magnitude there."""
    _bn_check(n, c, "contiguous", "contiguous")


@pytest.mark.parametrize("n", K.BN_ROWS)
@pytest.mark.parametrize("c", K.BN_LAYOUT_WIDTHS)
def test_batchnorm_strided_and_misaligned_inputs_agree_with_the_contiguous_call(n, c):
    """ld = c + 4 keeps the 16-byte paths on a strided view; ld = c + 1 and a base 4 bytes past a 16-byte boundary switch both
    the partial walk and the apply to their scalar forms.  x and dy take different layouts in the backward.  The walks associate
    the double sums differently, so the results agree within the bounds, not bitwise."""
    base, bounds = _bn_check(n, c, "contiguous", "contiguous")
    others = K.BN_LAYOUTS[1:]
    for i, lay_x in enumerate(others):
        for lay_dy in (others[(i + 1) % 3], "contiguous"):
            got, _ = _bn_check(n, c, lay_x, lay_dy)
            for k in got:
                assert _within(got[k], base[k].cpu().double(), bounds[k]) <= 1.0, (k, lay_x, lay_dy)


def test_batchnorm_wider_than_the_kernels_falls_back_to_torch_in_the_module_wrapper():
    """ops.batchnorm_fwd / _bwd keep raising beyond 512 channels; batch_norm(module, x) runs torch's batch_norm there: forward,
    backward and statistics against torch.nn.BatchNorm1d on the CPU at the tolerances of the kernel path's own test."""
    ops = _ops()
    from laplace_amd._lib import MiError
    from laplace_amd.model.encoder_decoder import batch_norm
    n, c = 300, 520
    g = t.Generator().manual_seed(n + c)
    x = t.randn(n, c, generator=g) * 2.0 + 3.0 * t.randn(1, c, generator=g)
    w = t.randn(n, c, generator=g)
    for wide in (513, c):
        xs = t.zeros(4, wide, device=DEV)
        with pytest.raises(MiError):
            ops.batchnorm_fwd(xs, None, None, None, None, 0.1, 1e-5, True)
        with pytest.raises(MiError):
            ops.batchnorm_bwd(xs, xs, None, t.zeros(wide, device=DEV), t.ones(wide, device=DEV))
    for momentum in (0.1, None):
        ref = t.nn.BatchNorm1d(c, momentum=momentum)
        with t.no_grad():
            ref.weight.copy_(t.rand(c, generator=g) + 0.5)
            ref.bias.copy_(t.randn(c, generator=g))
        mine = t.nn.BatchNorm1d(c, momentum=momentum)
        mine.load_state_dict(ref.state_dict())
        mine.to(DEV)
        for it in range(3):
            xr = x.clone().requires_grad_(True)
            xg = x.clone().to(DEV).requires_grad_(True)
            yr, yg = ref(xr), batch_norm(mine, xg)
            assert (yg.detach().cpu() - yr.detach()).abs().max() <= 2e-5
            ref.zero_grad(); mine.zero_grad()
            (yr * w).sum().backward()
            (yg * w.to(DEV)).sum().backward()
            scale = float(xr.grad.abs().max()) + 1e-6
            assert (xg.grad.cpu() - xr.grad).abs().max() <= 1e-4 * scale + 1e-6
            for a, b in ((mine.weight.grad, ref.weight.grad), (mine.bias.grad, ref.bias.grad)):
                assert (a.cpu() - b).abs().max() <= 1e-4 * (float(b.abs().max()) + 1.0)
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert t.allclose(getattr(mine, k).cpu().float(), getattr(ref, k).float(), rtol=1e-5, atol=1e-6), k
            assert int(mine.num_batches_tracked) == it + 1
        ref.eval(); mine.eval()
        before = {k: v.clone() for k, v in mine.state_dict().items()}
        assert (batch_norm(mine, x.to(DEV)).cpu() - ref(x)).abs().max() <= 2e-5
        for k, v in mine.state_dict().items():
            assert t.equal(v, before[k]), k                                          # eval mode leaves the statistics alone


# ------------------------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("n", K.BCE_SIZES)
def test_bce_logits_against_float64(n):
    """n around the single 1024-thread workgroup (one thread idle, every thread one element, one thread two), saturated logits,
    soft labels; want_grad=False; repeated calls."""
    ops = _ops()
    x, y = K.bce_case(n)
    ref = K.bce_ref(x, y)
    xg, yg = x.to(DEV), y.to(DEV)
    loss, dx = ops.bce_logits(xg, yg)
    e_loss = abs(float(loss.cpu().double()[0]) - float(ref["loss"])) / float(ref["loss_bound"])
    e_dx = _within(dx, ref["dx"], ref["dx_bound"])
    print(f"bce n={n} error/bound: loss={e_loss:.3f} dx={e_dx:.3f}")
    assert loss.shape == (1,) and dx.shape == (n,)
    assert e_loss <= 1.0 and e_dx <= 1.0
    loss_only, none = ops.bce_logits(xg, yg, want_grad=False)
    assert none is None and t.equal(loss_only, loss)
    for _ in range(2):
        l2, d2 = ops.bce_logits(xg, yg)
        assert t.equal(l2, loss) and t.equal(d2, dx)
    d = dx.cpu()
    assert bool(t.isfinite(d).all()) and bool(t.isfinite(loss).all())
    assert bool((d[y == 0] >= 0).all()) and bool((d[y == 1] <= 0).all())            # sigmoid(x) - y never leaves [-1, 1] - y
    if n > 1:
        for v, lab, want in ((100.0, 0.0, 1.0 / n), (-100.0, 1.0, -1.0 / n)):       # saturated against the label: the full +-1 / n
            sel = (x == v) & (y == lab)
            assert int(sel.sum()) == 1 and abs(float(d[sel]) - want) <= 8 * K.U / n
        for v, lab in ((100.0, 1.0), (-100.0, 0.0)):                                # saturated with the label: (signed) zero
            sel = (x == v) & (y == lab)
            assert int(sel.sum()) == 1 and abs(float(d[sel])) <= 8 * K.U / n


# ---------------------------------------------------------------------------------------------------------- embed_concat
@pytest.mark.parametrize("name", [c[0] for c in K.EMBED_CASES])
def test_embed_concat_wide_tables_against_float64(name):
    """Width 64: the last that fits the 16-lane instantiation's v[4]; 65, 128, 200 and [4, 130]: the whole-wavefront one;
    twenty columns: two launches into one strided output, the first (widths <= 8) 16-lane, the second (a width of 96) whole-
    wavefront.  Tables scaled to norms well below and well above max_norm = 1."""
    ops = _ops()
    tables, x = K.embed_case(name)
    want, bound, near = K.embed_ref(x, tables, 1.0)
    assert near == 0
    tg = [tb.to(DEV) for tb in tables]
    got = ops.embed_concat(x.to(DEV), tg, max_norm=1.0)
    assert got.shape == want.shape
    e = _within(got, want, bound)
    print(f"embed_concat {name} error/bound: {e:.3f}")
    assert e <= 1.0
    for tb, dev in zip(tables, tg):
        assert t.equal(dev.cpu(), tb)                                                # the lookup renormalises no table in place
    plain = ops.embed_concat(x.to(DEV), tg, max_norm=0.0)
    assert t.equal(plain.cpu(), t.cat([tb[x[:, i]] for i, tb in enumerate(tables)], 1))
    assert t.equal(ops.embed_concat(x.to(DEV), tg, max_norm=1.0), got)


# ------------------------------------------------------------------------------------------------------------ segment max
@pytest.mark.parametrize("n_dst", K.SEG_DSTS)
@pytest.mark.parametrize("d", K.SEG_WIDTHS)
def test_segment_max_ties_infinities_and_empty_segments(n_dst, d):
    """Exact ties (three identical source rows): arg names the smallest id and the backward gives it the whole gradient;
    all -inf segments; all-negative segments; empty first and last destination; duplicated edges; X and dY strided (ld = d + 3);
    n_dst = 1, 5, 203: not multiples of the 4 rows of a workgroup; d = 1 .. 129: one to three passes of the lane loop."""
    ops = _ops()
    src, dst, X, dY = K.segmax_case(n_dst, d)
    by_dst = ops.coo_to_csr(dst.to(DEV), src.to(DEV), n_dst, K.SEG_SRC, want_perm=False)
    by_src = ops.coo_to_csr(src.to(DEV), dst.to(DEV), K.SEG_SRC, n_dst, want_perm=False)
    want_y, want_arg = K.segmax_ref(src, dst, X, n_dst)
    Xg = _layout(X, "ld+3")
    Y, arg = ops.segment_max(by_dst, Xg)
    assert t.equal(Y.cpu().double(), want_y)
    assert t.equal(arg.cpu().long(), want_arg)
    assert not bool(((want_arg == 7) | (want_arg == 9)).any()) and bool((want_arg == 2).any())
    assert t.equal(ops.segment_max(by_dst, X.to(DEV), want_arg=False)[0], Y)         # contiguous X, no arg: the same maxima
    ref, bound = K.segmax_bwd_ref(want_arg, dY, K.SEG_SRC)
    dX = ops.segment_max_bwd(by_src, arg, _layout(dY, "ld+3"))
    e = _within(dX, ref, bound)
    print(f"segment_max_bwd n_dst={n_dst} d={d} error/bound: {e:.3f}")
    assert e <= 1.0
    assert bool((dX[7] == 0).all()) and bool((dX[9] == 0).all())                     # the later tied sources get nothing
    if n_dst == 5:   # destination 1 = {9, 7, 2} is the only segment holding source 2: its gradient row, whole and unrounded
        assert bool((want_arg[1] == 2).all()) and t.equal(dX[2].cpu(), dY[1])
    for _ in range(2):
        assert t.equal(ops.segment_max_bwd(by_src, arg, _layout(dY, "ld+3")), dX)
    assert t.equal(ops.segment_max_bwd(by_src, arg, dY.to(DEV)), dX)


# ------------------------------------------------------------------------------------------------------------ CSR builders
def _variants(n_rows):
    return ("largest", "empty_ends") if n_rows >= 3 else ("largest",)   # one or two rows cannot have an empty first and last row


@pytest.mark.parametrize("n_rows,n_cols", K.CSR_SHAPES)
def test_coo_to_csr_at_the_key_width_boundaries_with_the_stable_permutation(n_rows, n_cols):
    """Row and column counts at a power of two and one above it (where the packed key's field width changes) with the largest ids
    planted; rowptr, col and perm equal the oracle's — perm the STABLE one: duplicates carry distinct weights."""
    ops = _ops()
    for variant in _variants(n_rows):
        row, col = K.coo_case(n_rows, n_cols, variant)
        rowptr, col_s, perm = R.sparse_tensor_csr(row, col, n_rows, n_cols)
        a = ops.coo_to_csr(row.to(DEV), col.to(DEV), n_rows, n_cols)
        assert t.equal(a.rowptr.cpu().long(), rowptr), variant
        assert t.equal(a.col.cpu().long(), col_s), variant
        assert t.equal(a.perm.cpu().long(), perm), variant
        w = t.arange(row.numel(), dtype=t.float32) * 0.5 + 1.0
        assert t.equal(ops.gather_f32(w.to(DEV), a.perm).cpu(), w[perm])
        b = ops.coo_to_csr(row.to(DEV), col.to(DEV), n_rows, n_cols, want_perm=False)
        assert b.perm is None and t.equal(b.rowptr, a.rowptr) and t.equal(b.col, a.col)


@pytest.mark.parametrize("n_rows,n_cols", K.CSR_SHAPES)
def test_csr_transpose_rectangular_both_ways_with_the_stable_permutation(n_rows, n_cols):
    ops = _ops()
    for variant in _variants(n_rows) + ("nnz0",):
        if variant == "nnz0":
            row = col = t.zeros(0, dtype=t.int64)
        else:
            row, col = K.coo_case(n_rows, n_cols, variant)
            if n_cols >= 3:
                col = t.where(col == 1, t.zeros_like(col), col)                          # column 1 of A = row 1 of A^T is empty
        a = ops.coo_to_csr(row.to(DEV), col.to(DEV), n_rows, n_cols)
        rowptr, col_s, perm = R.sparse_tensor_csr(row, col, n_rows, n_cols)
        row_s = t.repeat_interleave(t.arange(n_rows), rowptr[1:] - rowptr[:-1])
        val = t.arange(row.numel(), dtype=t.float32) * 0.25 - 3.0
        a.val = val.to(DEV)
        at = ops.csr_transpose(a)
        rowptr_t, col_t, perm_t = R.sparse_tensor_csr(col_s, row_s, n_cols, n_rows)     # stable sort by (col, row)
        assert (at.n_rows, at.n_cols) == (n_cols, n_rows)
        assert t.equal(at.rowptr.cpu().long(), rowptr_t), variant
        assert t.equal(at.col.cpu().long(), col_t), variant
        assert t.equal(at.perm.cpu().long(), perm_t), variant
        assert t.equal(at.val.cpu(), val[perm_t]), variant
        if variant != "nnz0" and n_cols >= 3:
            assert int(rowptr_t[1]) == int(rowptr_t[2])


def _gappy_csr(seed=5):
    """30 x 17 CSR: rows 0-2, 9-13 and 27-29 empty (leading, interior and trailing runs), rows 5 and 20 long."""
    g = t.Generator().manual_seed(seed)
    live = t.tensor([r for r in range(3, 27) if not 9 <= r <= 13])
    row = live[t.randint(0, live.numel(), (300,), generator=g)]
    row = t.cat([row, t.full((80,), 5), t.full((70,), 20)])
    col = t.randint(0, 17, (row.numel(),), generator=g)
    return row, col, 30, 17


@pytest.mark.parametrize("n_rows,n_cols", K.CSR_SHAPES[2:] + ((30, 17),))
def test_scale_csr_and_expand_rows_exact(n_rows, n_cols):
    """scale_csr is two float32 multiplies in a fixed order — (v * row_scale[row]) * col_scale[col] — so it equals the CPU's
    float32 product bit for bit; expand_rows equals repeat_interleave.  Runs of empty rows at the start, inside and at the end
    (the binary search for an entry's row), and the aggr="mean" use: row_scale = 1 / in-degree with zero-degree rows."""
    ops = _ops()
    if (n_rows, n_cols) == (30, 17):
        row, col, n_rows, n_cols = _gappy_csr()
    else:
        row, col = K.coo_case(n_rows, n_cols, "empty_ends")
    a = ops.coo_to_csr(row.to(DEV), col.to(DEV), n_rows, n_cols)
    rowptr, col_s, _ = R.sparse_tensor_csr(row, col, n_rows, n_cols)
    deg = rowptr[1:] - rowptr[:-1]
    row_s = t.repeat_interleave(t.arange(n_rows), deg)
    assert int(deg[0]) == 0 and int(deg[-1]) == 0
    assert t.equal(ops.expand_rows(a).cpu().long(), row_s)
    g = t.Generator().manual_seed(n_rows + n_cols)
    v = t.randn(a.nnz, generator=g)
    rs, cs = t.randn(n_rows, generator=g), t.randn(n_cols, generator=g)
    one = t.ones(a.nnz)
    for val_in in (None, v):
        base = one if val_in is None else val_in
        vg = None if val_in is None else val_in.to(DEV)
        assert t.equal(ops.scale_csr(a, vg, rs.to(DEV), None).cpu(), base * rs[row_s])
        assert t.equal(ops.scale_csr(a, vg, None, cs.to(DEV)).cpu(), base * cs[col_s])
        assert t.equal(ops.scale_csr(a, vg, rs.to(DEV), cs.to(DEV)).cpu(), (base * rs[row_s]) * cs[col_s])
        assert t.equal(ops.scale_csr(a, vg, None, None).cpu(), base)
    degf = deg.float()
    inv = t.where(degf > 0, 1.0 / degf, t.zeros_like(degf))                              # model/layers.py, aggr="mean"
    mean_w = ops.scale_csr(a, None, inv.to(DEV), None).cpu()
    assert t.equal(mean_w, inv[row_s])
    sums = t.zeros(n_rows, dtype=t.float64).index_add_(0, row_s, mean_w.double())
    assert bool(((sums - (deg > 0).double()).abs() <= deg.double() * K.U).all())         # every non-empty row's weights sum to 1


# ------------------------------------------------------------------------------------------------------------ gather_cat
@pytest.mark.parametrize("cu,ci", [(1, 67), (64, 0), (0, 5)])
def test_gather_cat_forward_odd_widths_strided_and_repeated_rows(cu, ci):
    ops = _ops()
    g = t.Generator().manual_seed(cu * 100 + ci)
    nu, ni, ne = 9, 33, 1001
    zu, zi = t.randn(nu, cu, generator=g), t.randn(ni, ci, generator=g)
    row = t.randint(0, 3, (ne,), generator=g)                                            # three users named ~330 times each
    col = t.randint(0, ni, (ne,), generator=g)
    col[::5] = ni - 1
    row[-1] = nu - 1
    out = ops.gather_cat(_layout(zu, "ld+3"), zi.to(DEV), row.to(DEV), col.to(DEV))
    assert out.shape == (ne, cu + ci)
    assert t.equal(out.cpu(), t.cat([zu[row], zi[col]], dim=-1))
    assert t.equal(ops.gather_cat(zu.to(DEV), _layout(zi, "ld+1"), row.to(DEV), col.to(DEV)), out)
