"""Every launch form of the dense Adam update (mi_adam_dense_f32, mi_adam_multi_f32, mi_ranker_adam_f32, the SpMM optimizer
epilogue) and the row-copy kernels (mi_gather_rows_f32, mi_scatter_rows_f32) against the float32 restatements of
tests/adam_refs.py, bit for bit, and the float64 torch.optim.Adam twin at the bars of test_adam_matches_torch_optim.

Operands are carved out of one allocation per test that is filled with a NaN of a fixed payload; the whole allocation is compared
with its host mirror byte for byte afterwards, so padding columns, the guard floats around every tensor and rows outside a window
are checked together with the results."""
import ctypes

import numpy as np
import pytest
import torch as t

import adam_refs as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = np.uint32(0x7FD5A5A5)     # a quiet NaN with a payload no arithmetic produces
GUARD = 8                            # sentinel floats before and after every operand (a multiple of 4: keeps 16-byte alignment)


def _ops():
    from laplace_amd import ops
    return ops


def _L():
    from laplace_amd import _lib
    return _lib


class Arena:
    """Operands [rows, d] with leading dimension ld (vectors: rows = 1), `mis` floats past a 16-byte boundary, laid out in one
    buffer with GUARD sentinel floats around each; self.h is the host mirror (uint32)."""

    def __init__(self):
        self.n, self.slots, self.h = GUARD, {}, None

    def take(self, name, rows, d, ld=None, mis=0):
        assert self.h is None and name not in self.slots and self.n % 4 == 0
        ld = d if ld is None else ld
        start = self.n + mis
        self.slots[name] = (start, rows, d, ld)
        self.n = -(-(start + rows * ld) // 4) * 4 + GUARD
        return self

    def build(self):
        self.h = np.full(self.n, SENTINEL, dtype=np.uint32)
        return self

    def host(self, name, buf=None):
        start, rows, d, ld = self.slots[name]
        buf = self.h if buf is None else buf
        return buf.view(F)[start:start + rows * ld].reshape(rows, ld)[:, :d]

    def upload(self):
        dev = t.from_numpy(self.h.view(np.int32)).to(DEV)
        assert dev.data_ptr() % 16 == 0
        return dev

    def dev(self, buf, name):
        start, rows, d, ld = self.slots[name]
        return buf.view(t.float32)[start:start + rows * ld].view(rows, ld)[:, :d]

    def ptr(self, buf, name):
        start, rows, d, _ = self.slots[name]
        return buf.data_ptr() + 4 * start if rows * d else None

    @staticmethod
    def download(buf):
        t.cuda.synchronize()
        return buf.cpu().numpy().view(np.uint32)

    def where(self, i):
        for name, (start, rows, d, ld) in self.slots.items():
            if start <= i < start + rows * ld:
                r, c = divmod(i - start, ld)
                return f"{name}[{r}, {c}]" + (" (padding column)" if c >= d else "")
        return "a guard float"

    def same(self, got, want, what=""):
        """Byte equality of two images of the arena; names the first float that differs."""
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} floats differ, first at {self.where(i)}: "
                             f"got {got[i]:#010x} ({got.view(F)[i]!r}), want {want[i]:#010x} ({want.view(F)[i]!r})")


def _fractions(got, ref):
    return {k: A.bar_fraction(x, y, k) for k, x, y in zip("pmv", got, ref)}


def _within_bars(tag, got, ref):
    fr = _fractions(got, ref)
    print(f"{tag}: worst fraction of the bars p {fr['p']:.3g} m {fr['m']:.3g} v {fr['v']:.3g}")
    assert max(fr.values()) <= 1.0, fr


# ------------------------------------------------------------------------------------------------- a. mi_adam_dense_f32
def _dense(case, hyper, step, seed):
    ops = _ops()
    d, n, strided = case["d"], case["n_rows"], case["strided"]
    ar = Arena()
    ar.take("p", n, d, d + A.DENSE_PAD_P if strided else d).take("g", n, d, d + A.DENSE_PAD_G if strided else d)
    ar.take("m", n, d).take("v", n, d).take("w", 1, n).build()
    p, g, m, v = A.state((n, d), seed)
    w = (np.random.default_rng(seed + 1).random(n) * 1e-3).astype(F) if case["reg_w"] else None
    for name, x in zip("pgmv", (p, g, m, v)):
        ar.host(name)[:] = x
    if w is not None:
        ar.host("w")[0] = w
    images = []
    for _ in range(2):                                           # the same call twice from the same state: the same bits
        buf = ar.upload()
        ops.adam_step(ar.dev(buf, "p"), ar.dev(buf, "g"), ar.dev(buf, "m"), ar.dev(buf, "v"), step=step, lr=hyper[0],
                      beta1=hyper[1], beta2=hyper[2], eps=hyper[3], reg_w=ar.dev(buf, "w")[0] if w is not None else None)
        images.append(ar.download(buf))
        del buf
    want = ar.h.copy()
    ref = A.update(p, g, m, v, A.constants(*hyper, step), reg_w=w)
    for name, x in zip("pmv", ref):
        ar.host(name, want)[:] = x
    ar.same(images[0], want, "against update()")
    ar.same(images[1], images[0], "second call")
    got = [ar.host(name, images[0]) for name in "pmv"]
    if w is None:                                                # zero gradient and zero moments: the parameter's bits stay
        still = A.still_mask((n, d))
        assert np.array_equal(got[0][still].view(np.uint32), p[still].view(np.uint32))
    assert not np.array_equal(got[0], p)
    _within_bars(f"dense {case} step {step}", got, A.twin_f64(p, g, m, v, hyper, step, reg_w=w))


def _case_id(c):
    return f"d{c['d']}-n{c['n_rows']}" + ("-reg_w" if c["reg_w"] else "") + ("-strided" if c["strided"] else "")


@pytest.mark.parametrize("case", A.DENSE_CASES, ids=_case_id)
def test_adam_dense_every_lane_layout(case):
    """Idle lanes (d = 12, 200, 260), a column loop of two and three trips (1028, 2052), row counts around one block's rows,
    padding columns of p and the gradient, with and without the per-row L2 weight."""
    _dense(case, A.HYPERS[0], 3, seed=case["d"] + case["n_rows"])


def test_adam_dense_grid_stride_second_pass():
    """More rows than the capped grid takes in one pass: the last 300 are the stride loop's second trip.  Every row checked."""
    _dense(A.GRID_CAP_CASE, A.HYPERS[0], 2, seed=77)


@pytest.mark.parametrize("step", A.STEPS)
@pytest.mark.parametrize("hyper", A.HYPERS)
def test_adam_dense_hyperparameters_and_steps(hyper, step):
    n, d = A.HYPER_SHAPE
    _dense(dict(d=d, n_rows=n, reg_w=True, strided=True), hyper, step, seed=step % 1000)
    _dense(dict(d=d, n_rows=n, reg_w=False, strided=False), hyper, step, seed=step % 1000 + 5)


# ------------------------------------------------------------------------------------------------ b. mi_adam_multi_f32
def _tensor_list(sizes, mis=None):
    """Arena with p/g/m/v of every tensor, states filled in; returns (arena, [state per tensor])."""
    ar = Arena()
    for i, n in enumerate(sizes):
        for k in "pgmv":
            ar.take(f"{k}{i}", 1, n, mis=mis[i][k] if mis else 0)
    ar.build()
    states = []
    for i, n in enumerate(sizes):
        st = A.state((n,), seed=1000 + i)
        for k, x in zip("pgmv", st):
            ar.host(f"{k}{i}")[0] = x
        states.append(st)
    return ar, states


def _param_array(ar, buf, count, params, null_empty=True):
    L = _L()
    for i in range(count):
        n = ar.slots[f"p{i}"][2]
        for k in "pgmv":   # an empty tensor: null pointers (mi_adam_multi_f32), or any valid address (mi_ranker_adam_f32)
            setattr(params[i], k, ar.ptr(buf, f"{k}{i}") if n or null_empty else buf.data_ptr())
        params[i].n = n
    return L


def _expect(ar, states, consts, g_scale=1.0):
    want = ar.h.copy()
    refs = []
    for i, (p, g, m, v) in enumerate(states):
        ref = A.update(p, g, m, v, consts, g_scale=g_scale)
        for k, x in zip("pmv", ref):
            ar.host(f"{k}{i}", want)[0] = x
        refs.append(ref)
    return want, refs


def _twin_all(tag, ar, image, states, hyper, step, g_scale=1.0):
    live = [i for i, s in enumerate(states) if s[0].size]
    cat = [np.concatenate([states[i][j] for i in live]) for j in range(4)]
    got = [np.concatenate([ar.host(f"{k}{i}", image)[0] for i in live]) for k in "pmv"]
    _within_bars(tag, got, A.twin_f64(*cat, hyper, step, g_scale=g_scale))


@pytest.mark.parametrize("name", list(A.MULTI_LISTS))
def test_adam_multi_dispatch(name):
    """The dispatcher's four rules: the dense kernel for a large aligned tensor, the table for everything else (large and
    misaligned in several grid passes, large and no multiple of 4), a table flushed at 48 tensors, empty tensors skipped."""
    entries = A.MULTI_LISTS[name]
    hyper, step = A.HYPERS[1], 7
    ar, states = _tensor_list([e["n"] for e in entries], [e["mis"] for e in entries])
    buf = ar.upload()
    params = (_L().RankerParam * len(entries))()
    L = _param_array(ar, buf, len(entries), params)
    for i, e in enumerate(entries):
        for k in "pgmv":
            q = getattr(params[i], k)
            assert (q is None) == (e["n"] == 0) and (q is None or q % 16 == 4 * e["mis"][k])
    assert L.lib().mi_adam_multi_f32(params, len(entries), *hyper, step, L.current_stream()) == 0
    got = ar.download(buf)
    want, _ = _expect(ar, states, A.constants(*hyper, step))
    ar.same(got, want, "against update()")
    for i, (p, _, _, _) in enumerate(states):
        still = A.still_mask(p.shape)
        assert np.array_equal(ar.host(f"p{i}", got)[0][still].view(np.uint32), p[still].view(np.uint32))
    _twin_all(f"multi {name}", ar, got, states, hyper, step)
    assert L.lib().mi_adam_multi_f32(None, 0, *hyper, step, L.current_stream()) == 0
    ar.same(ar.download(buf), got, "n_params = 0")


# ----------------------------------------------------------------------------------------------- c. mi_ranker_adam_f32
def _ranker_model(ar, buf, n_params, hyper, step):
    L = _L()
    model = L.RankerModel()                                     # everything the function does not read stays zero
    _param_array(ar, buf, min(n_params, len(ar.slots) // 4), model.params, null_empty=False)
    model.n_params = n_params
    model.lr, model.beta1, model.beta2, model.eps = hyper
    model.step = step
    return L, model


@pytest.mark.parametrize("n_params", [1, 48])
@pytest.mark.parametrize("g_scale", A.RANKER_GRAD_SCALES, ids=lambda s: f"scale{s:.3g}")
def test_ranker_adam_scales_the_gradient_first(g_scale, n_params):
    hyper, step = A.HYPERS[0], 7
    sizes = A.RANKER_SIZES if n_params == 48 else (A.RANKER_SIZES[5],)
    ar, states = _tensor_list(sizes)
    buf = ar.upload()
    L, model = _ranker_model(ar, buf, n_params, hyper, step)
    assert L.lib().mi_ranker_adam_f32(ctypes.byref(model), g_scale, L.current_stream()) == 0
    got = ar.download(buf)
    want, _ = _expect(ar, states, A.constants(*hyper, step), g_scale=g_scale)
    ar.same(got, want, "against update(g_scale=)")
    _twin_all(f"ranker adam scale {g_scale:.3g} n_params {n_params}", ar, got, states, hyper, step, g_scale=g_scale)


def test_ranker_adam_step_zero_empty_list_and_bad_arguments():
    hyper = A.HYPERS[2]
    sizes = (257, 0, 3)
    ar, states = _tensor_list(sizes)
    images = []
    for step in (0, 1):                                         # a model that never stepped: step 0 is read as 1
        buf = ar.upload()
        L, model = _ranker_model(ar, buf, len(sizes), hyper, step)
        assert L.lib().mi_ranker_adam_f32(ctypes.byref(model), 1.0, L.current_stream()) == 0
        images.append(ar.download(buf))
    want, _ = _expect(ar, states, A.constants(*hyper, 1))
    ar.same(images[1], want, "step 1 against update()")
    ar.same(images[0], images[1], "step 0 against step 1")
    buf = ar.upload()
    for n_params, g_scale, rc in ((0, 1.0, 0), (49, 1.0, L.MI_ERR_BAD_ARG), (len(sizes), 0.0, L.MI_ERR_BAD_ARG)):
        L, model = _ranker_model(ar, buf, n_params, hyper, 1)
        assert L.lib().mi_ranker_adam_f32(ctypes.byref(model), g_scale, L.current_stream()) == rc, (n_params, g_scale)
    ar.same(ar.download(buf), ar.h, "calls that must write nothing")


# ------------------------------------------------------------------------------------------ d. the SpMM optimizer epilogue
def test_spmm_adam_epilogue_is_update_of_its_own_gradient():
    """The fused form against the restatement directly: p, m, v of spmm(adam=) are update() of the S the same call returns."""
    ops = _ops()
    n, n_cols, d, hyper, step = 300, 500, 200, A.HYPERS[0], 7
    g = t.Generator().manual_seed(31)
    row = t.cat([t.full((700,), 41), t.randint(0, n, (6000,), generator=g)])
    row[row == 17] = 18                                          # a row without entries still gets its update
    col = t.randint(0, n_cols, (row.numel(),), generator=g)
    a = ops.coo_to_csr(row.to(DEV), col.to(DEV), n, n_cols, want_perm=False)
    a.val = (t.rand(a.nnz, generator=g) - 0.3).to(DEV)
    assert a.nnz < ops.PLAN_MIN_NNZ
    X, addend = t.randn(n_cols, d, generator=g).to(DEV), t.randn(n, d, generator=g).to(DEV)
    ar = Arena().take("p", n, d).take("m", n, d).take("v", n, d).take("S", n, d).take("w", 1, n).build()
    p, _, m, v = A.state((n, d), seed=32)
    w = (np.random.default_rng(33).random(n) * 1e-3).astype(F)
    for name, x in (("p", p), ("m", m), ("v", v)):
        ar.host(name)[:] = x
    ar.host("w")[0] = w
    buf = ar.upload()
    ops.spmm(a, X, addend=addend, S=ar.dev(buf, "S"), scale=0.25,
             adam=dict(p=ar.dev(buf, "p"), m=ar.dev(buf, "m"), v=ar.dev(buf, "v"), step=step, lr=hyper[0], beta1=hyper[1],
                       beta2=hyper[2], eps=hyper[3], reg_w=ar.dev(buf, "w")[0]))
    assert a.plan is None
    got = ar.download(buf)
    G = ar.host("S", got).copy()
    assert np.isfinite(G).all() and G[17].any()
    want = ar.h.copy()                # (a launch without adam= sums the 730-entry row cooperatively: another order, other bits)
    ar.host("S", want)[:] = G
    for name, x in zip("pmv", A.update(p, G, m, v, A.constants(*hyper, step), reg_w=w)):
        ar.host(name, want)[:] = x
    ar.same(got, want, "against update() of S")
    _within_bars("spmm epilogue", [ar.host(k, got) for k in "pmv"], A.twin_f64(p, G, m, v, hyper, step, reg_w=w))


# -------------------------------------------------------------------------------------- e. gather_rows / scatter_rows
def _i32(x):
    return None if x is None else t.tensor([x], dtype=t.int32, device=DEV)


@pytest.mark.parametrize("case", A.ROW_COPY_CASES, ids=lambda c: f"d{c['d']}" + ("-strided" if c["strided"] else "") + f"-off{c['row_offset']}")
def test_gather_and_scatter_rows_windows(case):
    """Both kernels over every window form, gather with every (accumulate, scale); rows outside the window, padding columns
    and guards keep their sentinel bytes; scatter then gather over one window restores the source rows."""
    ops = _ops()
    d, off = case["d"], case["row_offset"]
    ld = d + 4 if case["strided"] else d
    n, n_table = A.ROW_COPY_N, A.ROW_COPY_TABLE
    rng = np.random.default_rng(d + off)
    rows_h = (rng.permutation(n_table)[:n] + off).astype(np.int32)
    rows = t.from_numpy(rows_h).to(DEV)
    table_h = rng.standard_normal((n_table, d)).astype(F)
    small_h = rng.standard_normal((n, d)).astype(F)
    old_h = rng.standard_normal((n, d)).astype(F)
    for wname, (begin, n_end) in A.ROW_COPY_WINDOWS.items():
        lo, hi = A.window(n, begin, n_end)
        kw = dict(n_dev=_i32(n_end), begin_dev=_i32(begin), row_offset=off)
        # gather: table -> dst
        for accumulate, scale in A.ROW_COPY_MODES:
            ar = Arena().take("src", n_table, d, ld).take("dst", n, d, ld).build()
            ar.host("src")[:] = table_h
            if accumulate:
                ar.host("dst")[lo:hi] = old_h[lo:hi]            # read inside the window only: the rest stays sentinel
            buf = ar.upload()
            ops.gather_rows(ar.dev(buf, "dst"), ar.dev(buf, "src"), rows, accumulate=accumulate, scale=scale, **kw)
            want = ar.h.copy()
            A.gather_rows_ref(ar.host("dst", want), ar.host("src", want), rows_h, off, begin, n_end, accumulate, scale)
            ar.same(ar.download(buf), want, f"gather {wname} accumulate={accumulate} scale={scale}")
        # scatter: src -> table, then gather it back
        ar = Arena().take("src", n, d, ld).take("table", n_table, d, ld).take("back", n, d, ld).build()
        ar.host("src")[:] = small_h
        buf = ar.upload()
        ops.scatter_rows(ar.dev(buf, "table"), ar.dev(buf, "src"), rows, **kw)
        want = ar.h.copy()
        A.scatter_rows_ref(ar.host("table", want), ar.host("src", want), rows_h, off, begin, n_end)
        got = ar.download(buf)
        ar.same(got, want, f"scatter {wname}")
        ops.gather_rows(ar.dev(buf, "back"), ar.dev(buf, "table"), rows, **kw)
        ar.host("back", want)[lo:hi] = small_h[lo:hi]
        ar.same(ar.download(buf), want, f"scatter then gather {wname}")
        assert int((ar.host("table", want).view(np.uint32)[:, 0] != SENTINEL).sum()) == hi - lo
