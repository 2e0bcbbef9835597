"""GPU: every tile kernel and K slicing the GEMM dispatcher can pick (csrc/gemm.hip: gemm_f32_kernel, the four
gemm_fast_kernel instantiations, gemm_group_kernel, the two slab reduces), on the case table of tests/gemm_cases.py.  For each
case: the launcher's own decision function, asked on the pointers the call gets, says the call takes the kernel / slicing /
share-set layout the case was written for; every output element equals the reference bit for bit (one k-ascending fma chain, or
the slab association of the reduce kernels: gemm_cases.py); it is within the derived bound of the float64 product; a second call
returns the same bits; C outside the written columns and the operands are untouched.  Calls go through the raw binding, so
leading dimensions, offsets and the workspace are exactly the case's.  tests/test_gemm_cases_cpu.py checks the same table's
branches and coverage without a GPU.  Below the table: calls the grouped entry declines (nothing may be written), and
mi_sage_wgrad_f32 with four problems in one call, a fifth declined, and non-finite dy behind a closed mask."""
import ctypes
import os
import sys

import pytest
import torch as t

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(x):
    return x.contiguous().view(t.int32)


def _same_bits(x, y):
    """Bitwise, NaN padding included."""
    return t.equal(_bits(x.cpu()), _bits(y.cpu()))


def _ratio(got, rec):
    """Largest |got - float64| / bound over the elements with a non-zero bound; asserts the bound."""
    err = (got.double() - rec["exact"]).abs()
    assert bool((err <= rec["bound"]).all())
    nz = rec["bound"] > 0
    return float((err[nz] / rec["bound"][nz]).max()) if bool(nz.any()) else 0.0


def _ws(nbytes):
    return t.empty(max(int(nbytes), 256), dtype=t.uint8, device=DEV)


@pytest.mark.parametrize("case", G.SINGLE, ids=lambda c: c.name)
def test_single_case_runs_its_declared_kernel_and_equals_the_reference(case):
    from laplace_amd import _lib
    L, c = _lib.lib(), case
    d = G.make_single(c)
    a_buf, b_buf = d["a_buf"].to(DEV), d["b_buf"].to(DEV)
    bias = d["bias"].to(DEV) if c.bias else None
    assert a_buf.data_ptr() % 256 == 0 and b_buf.data_ptr() % 256 == 0
    pa, lda, pb, ldb = G.single_addresses(c, a_buf.data_ptr(), b_buf.data_ptr())
    ws_bytes = int(L.mi_gemm_workspace_bytes(c.m, c.n, c.k))
    ws = _ws(ws_bytes)
    # 1. the decision: asked of the function the launcher calls, on the pointers the call gets
    info = _lib.GemmPlanInfo()
    assert L.mi_gemm_plan(int(c.trans_a), int(c.trans_b), c.m, c.n, c.k, pa, lda, pb, ldb, 0, ws_bytes, ctypes.byref(info)) == 0
    assert (info.kernel, info.splits, info.k_per_split) == (c.kernel, c.splits, d["kps"] if c.splits > 1 else c.k), G.KERNEL_NAMES[info.kernel]

    def call(with_ws=True):
        out = d["c_full"].to(DEV)                                  # NaN wherever nothing is to be accumulated
        rc = L.mi_gemm_f32(int(c.trans_a), int(c.trans_b), c.m, c.n, c.k, pa, lda, pb, ldb, bias.data_ptr() if c.bias else None,
                           out.data_ptr(), c.ldc, int(c.accumulate), int(c.relu), ws.data_ptr() if with_ws else None,
                           ws_bytes if with_ws else 0, _lib.current_stream())
        assert rc == 0
        return out
    # 2. every element bit for bit, 3. within the derived bound of float64, 4. the same bits again
    out = call()
    got = out[:, :c.n].cpu()
    assert t.equal(got, d["want"]), f"{int((got != d['want']).sum())} of {got.numel()} elements differ"
    print(f"ratio {G.KERNEL_NAMES[c.kernel]} splits {c.splits}: {_ratio(got, d):.4f}")
    assert _same_bits(call(), out)
    assert bool(t.isnan(out[:, c.n:]).all())                       # the columns beside a column slice are not written
    assert _same_bits(a_buf, d["a_buf"]) and _same_bits(b_buf, d["b_buf"])
    # the short-workspace fallback: without a workspace the same call is the single chain
    if c.splits > 1:
        alone = call(with_ws=False)[:, :c.n].cpu()
        assert t.equal(alone, d["single_chain"]) and not t.equal(alone, got)


def _upload(gr, data):
    dev = {name: buf.to(DEV) for name, buf in data["buffers"].items()}
    for i, (p, r) in enumerate(zip(gr.probs, data["probs"])):
        dev[f"c{i}"] = r["c_full"].to(DEV)
        if p.bias:
            dev[f"bias{i}"] = r["bias_t"].to(DEV)
    return dev


def _problems(gr, dev):
    from laplace_amd import _lib
    addr = lambda name: dev[name].data_ptr() if dev[name].numel() else None
    return G.fill_problems((_lib.GemmProblem * len(gr.probs))(), gr, addr)


def _launch_group(arr, n):
    from laplace_amd import _lib
    L = _lib.lib()
    ws_bytes = int(L.mi_gemm_group_workspace_bytes(arr, n))
    ws = _ws(ws_bytes)
    return int(L.mi_gemm_group_f32(arr, n, ws.data_ptr(), ws_bytes, _lib.current_stream()))


@pytest.mark.parametrize("group", G.GROUPS, ids=lambda g: g.name)
def test_grouped_case_gets_its_declared_layout_and_equals_the_reference(group):
    from laplace_amd import _lib
    L, n = _lib.lib(), len(group.probs)
    data = G.make_group(group)
    dev = _upload(group, data)
    arr = _problems(group, dev)
    plan = (_lib.GemmGroupPlanInfo * n)()
    assert L.mi_gemm_group_plan(arr, n, plan) == 0
    assert [(o.launch, o.splits, o.k_per_split, o.share_set, o.first_wg, o.n_wg) for o in plan] == G.declared_group_plan(group)
    assert _launch_group(arr, n) == 0
    worst = 0.0
    for i, (p, r) in enumerate(zip(group.probs, data["probs"])):
        out = dev[f"c{i}"]
        got = out[:, :p.n].cpu()
        assert bool(t.isfinite(got).all()), i
        assert t.equal(got, r["want"]), f"problem {i}: {int((got != r['want']).sum())} of {got.numel()} elements differ"
        if got.numel():
            worst = max(worst, _ratio(got, r))
        assert bool(t.isnan(out[:, p.n:]).all()), i
    print(f"ratio grouped {group.name}: {worst:.4f}")
    for name, buf in data["buffers"].items():                       # operands and masks were not written to
        assert _same_bits(dev[name], buf), name
    # the same call again on fresh outputs: the same bits
    dev2 = dict(dev)
    for i, r in enumerate(data["probs"]):
        dev2[f"c{i}"] = r["c_full"].to(DEV)
    assert _launch_group(_problems(group, dev2), n) == 0
    for i in range(n):
        assert _same_bits(dev2[f"c{i}"], dev[f"c{i}"]), i


@pytest.mark.parametrize("where,what", [(1, "a_mask"), (9, "a_mask"), (9, "A"), (10, "lda2"), (3, "B")])
def test_a_call_with_one_unaligned_operand_is_declined_whole_and_writes_nothing(where, what):
    """Eleven problems, the first of them accumulating: one operand (or the mask) of one problem off its 16-byte grid, in the
    first launch of eight or in the second, declines the call before anything is enqueued — a caller that falls back to single
    calls must not find an `accumulate` output already added to."""
    from laplace_amd import _lib
    gr = G.Group("declined", (G.Prob(40, 24, 64, False, True, "sa", accumulate=True),) + tuple(
        G.Prob(65, 33, 76, False, False, f"a{i}", mask=f"m{i}", k2=36 if i == 10 else 0) for i in range(1, 11)))
    data = G.make_group(gr)
    dev = _upload(gr, data)
    arr = _problems(gr, dev)
    assert _lib.lib().mi_gemm_group_supported(arr, 11) == 1
    setattr(arr[where], what, getattr(arr[where], what) + (1 if what.startswith("ld") else 4))
    assert _lib.lib().mi_gemm_group_supported(arr, 11) == 0
    plan = (_lib.GemmGroupPlanInfo * 11)()
    assert _lib.lib().mi_gemm_group_plan(arr, 11, plan) == _lib.MI_ERR_UNSUPPORTED
    assert _launch_group(arr, 11) == _lib.MI_ERR_UNSUPPORTED
    t.cuda.synchronize()
    for i, r in enumerate(data["probs"]):
        assert _same_bits(dev[f"c{i}"], r["c_full"]), i


# ---- mi_sage_wgrad_f32 (csrc/wgrad.hip) -------------------------------------------------------------------------------------------
def _wgrad_problem(k, m, n1, n2, bias, mask, g, poison=False):
    dy = t.randn(k, m, device=DEV, generator=g)
    mk = t.randn(k, m, device=DEV, generator=g) if mask else None
    if poison:                                                       # closed entries: 0.0, -0.0, negative; dy non-finite behind them
        flat_m, flat_d = mk.view(-1), dy.view(-1)
        flat_m[0::5] = 0.0
        flat_m[1::5] = -0.0
        closed = (flat_m <= 0).nonzero().view(-1)
        flat_d[closed[0::3]] = float("inf")
        flat_d[closed[1::3]] = float("nan")
        flat_d[closed[2::3]] = -float("inf")
    b1 = t.randn(k, n1, device=DEV, generator=g)
    b2 = t.randn(k, n2, device=DEV, generator=g) if n2 else None
    return dict(dy=dy, mask=mk, b1=b1, b2=b2)


def _wgrad_outputs(p, bias):
    m, n1 = p["dy"].shape[1], p["b1"].shape[1]
    nan = lambda *s: t.full(s, float("nan"), device=DEV)
    return dict(p, gw1=nan(m, n1), gb=nan(m) if bias else None, gw2=nan(m, p["b2"].shape[1]) if p["b2"] is not None else None)


def _wgrad_check(p, k):
    """Against float64 with the bound of test_sage_wgrad_matches_the_three_products; the mask selects."""
    a = (t.where(p["mask"] > 0, p["dy"], t.zeros((), device=DEV)) if p["mask"] is not None else p["dy"]).double()
    assert bool(t.isfinite(a).all())
    for got, want in ((p["gw1"], a.t() @ p["b1"].double()), (p["gb"], a.sum(0) if p["gb"] is not None else None),
                      (p["gw2"], a.t() @ p["b2"].double() if p["b2"] is not None else None)):
        if want is None:
            continue
        assert bool(t.isfinite(got).all())
        scale = float(want.abs().max()) + 1e-12
        assert float((got.double() - want).abs().max()) <= 2e-6 * scale * max(1.0, (k / 1000) ** 0.5), (got.shape,)


def test_sage_wgrad_four_problems_in_one_call_and_a_fifth_declined():
    from laplace_amd import ops
    g = t.Generator(device=DEV).manual_seed(4)
    spec = [(700, 32, 37, 84, True, True), (1301, 64, 84, 0, True, False), (257, 96, 76, 200, False, True), (2049, 128, 128, 76, True, False)]
    ins = [_wgrad_problem(k, m, n1, n2, bias, mask, g) for k, m, n1, n2, bias, mask in spec]
    one, two = ([_wgrad_outputs(p, s[4]) for p, s in zip(ins, spec)] for _ in range(2))
    assert ops.sage_wgrad(one) and ops.sage_wgrad(two)
    for p, q, s in zip(one, two, spec):
        _wgrad_check(p, s[0])
        for key in ("gw1", "gb", "gw2"):
            assert (p[key] is None) == (q[key] is None)
            if p[key] is not None:
                assert t.equal(p[key], q[key]), key                   # bitwise repeatable
    # each problem alone gives the bits it gives in the call of four
    for p, s, ref in zip(ins, spec, one):
        alone = _wgrad_outputs(p, s[4])
        assert ops.sage_wgrad([alone])
        assert all(alone[key] is None or t.equal(alone[key], ref[key]) for key in ("gw1", "gb", "gw2"))
    # five problems: declined, by the wrapper and by the entry itself, nothing written
    from laplace_amd import _lib
    five = [_wgrad_outputs(p, s[4]) for p, s in zip(ins, spec)] + [_wgrad_outputs(ins[0], True)]
    assert not ops.sage_wgrad(five)
    arr = (_lib.WgradProblem * 5)()
    for q, s in zip(arr, five):
        q.k, q.m, q.n1, q.n2 = s["dy"].shape[0], s["dy"].shape[1], s["b1"].shape[1], s["b2"].shape[1] if s["b2"] is not None else 0
        q.dy, q.mask, q.b1, q.b2 = ops._ptr(s["dy"]), ops._ptr(s["mask"]), ops._ptr(s["b1"]), ops._ptr(s["b2"])
        q.gw1, q.gb, q.gw2 = ops._ptr(s["gw1"]), ops._ptr(s["gb"]), ops._ptr(s["gw2"])
    L = _lib.lib()
    assert L.mi_sage_wgrad_supported(arr, 5) == 0 and L.mi_sage_wgrad_supported(arr, 4) == 1
    ws = _ws(1 << 26)
    assert L.mi_sage_wgrad_f32(arr, 5, ws.data_ptr(), ws.numel(), _lib.current_stream()) == _lib.MI_ERR_UNSUPPORTED
    t.cuda.synchronize()
    for s in five:
        assert all(s[key] is None or bool(t.isnan(s[key]).all()) for key in ("gw1", "gb", "gw2"))


@pytest.mark.parametrize("k,m,n1,n2", [(129, 32, 4, 0), (700, 64, 84, 76), (1301, 96, 37, 200), (2049, 128, 128, 128)])
def test_sage_wgrad_mask_selects_non_finite_dy_behind_a_closed_entry_stays_out(k, m, n1, n2):
    """dy = inf / NaN where mask is 0.0, -0.0 or negative: the kernel reads dy as 0 there (a select, not a product with 0)."""
    from laplace_amd import ops
    g = t.Generator(device=DEV).manual_seed(k + m)
    ins = _wgrad_problem(k, m, n1, n2, True, True, g, poison=True)
    assert not bool(t.isfinite(ins["dy"]).all())
    p, p2 = _wgrad_outputs(ins, True), _wgrad_outputs(ins, True)
    assert ops.sage_wgrad([p]) and ops.sage_wgrad([p2])
    _wgrad_check(p, k)
    for key in ("gw1", "gb", "gw2"):
        assert p[key] is None or t.equal(p[key], p2[key])
