"""The references of tests/adam_refs.py against independent arithmetic, on a machine without a GPU: the float32 restatement of
mi_adam_update4 against a float64 torch.optim.Adam and against the float32 torch.optim.Adam, its exact fma against rational
arithmetic, its constants against decimal arithmetic, and the case tables against a restatement of the dispatcher's rule."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest
import torch as t

import adam_refs as A

F = np.float32


def _report(tag, fr):
    print(f"{tag}: worst fraction of the bars p {fr['p']:.3g} m {fr['m']:.3g} v {fr['v']:.3g}")


def _fractions(got, ref):
    return {k: A.bar_fraction(x, y, k) for k, x, y in zip("pmv", got, ref)}


# ------------------------------------------------------------------------------------------------- update vs the float64 twin
@pytest.mark.parametrize("reg_w", [False, True])
@pytest.mark.parametrize("hyper", A.HYPERS)
def test_update_is_within_the_bars_of_the_float64_twin(hyper, reg_w):
    """One step from a shared float32 state, every step count; a seventh of the gradient exactly zero."""
    p, g, m, v = A.state((64, 52), seed=11)
    w = (np.random.default_rng(5).random(64) * 1e-3).astype(F) if reg_w else None
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step in A.STEPS:
        got = A.update(p, g, m, v, A.constants(*hyper, step), reg_w=w)
        fr = _fractions(got, A.twin_f64(p, g, m, v, hyper, step, reg_w=w))
        worst = {k: max(worst[k], fr[k]) for k in worst}
        assert max(fr.values()) <= 1.0, (step, fr)
        if not reg_w:   # zero gradient, zero moments: the parameter keeps its bits
            still = A.still_mask(p.shape)
            assert still.any() and np.array_equal(got[0][still].view(np.uint32), p[still].view(np.uint32))
            assert not got[1][still].any() and not got[2][still].any()
    _report(f"update vs twin {hyper} reg_w={reg_w}", worst)


@pytest.mark.parametrize("g_scale", [0.5, 1.0 / 3.0])
def test_update_scales_the_gradient_first(g_scale):
    p, g, m, v = A.state((300,), seed=12)
    got = A.update(p, g, m, v, A.constants(*A.HYPERS[0], 7), g_scale=g_scale)
    fr = _fractions(got, A.twin_f64(p, g, m, v, A.HYPERS[0], 7, g_scale=g_scale))
    _report(f"update vs twin g_scale={g_scale:.3g}", fr)
    assert max(fr.values()) <= 1.0
    same = A.update(p, g * F(g_scale), m, v, A.constants(*A.HYPERS[0], 7))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, same))
    assert not np.array_equal(got[0], A.update(p, g, m, v, A.constants(*A.HYPERS[0], 7))[0])


# ------------------------------------------------------------------------------------------------------------ the exact fma
def _round_f32(x: Fraction) -> np.float32:
    """Fraction -> float32, round to nearest, ties to even, by exact comparison of the candidates."""
    near = F(float(x))                      # float(Fraction) is correctly rounded: near is one of the two neighbours or next to them
    cand = sorted({near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(-np.inf))}, key=float)
    cand = [c for c in cand if np.isfinite(c)]
    best = min(cand, key=lambda c: (abs(Fraction(float(c)) - x), int(np.array(c).view(np.uint32)) & 1))
    return best


def _exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def test_fma_matches_rational_arithmetic_on_random_triples():
    rng = np.random.default_rng(3)
    n = 4000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(F)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F)
    c[::5] = (-(a[::5].astype(np.float64) * b[::5].astype(np.float64))).astype(F)   # heavy cancellation: the low product bits decide
    c[1::50] = 0.0
    got = A.fma_f32(a, b, c)
    want = np.array([_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F)
    assert np.array_equal(_bits(got), _bits(want))


def _tie_triples():
    """(a, b, c, residual sign): a * b = -+(2^t - 2^(t-46)), c = +-(2^(t+24) + k * 2^(t+1)): the float64 sum a * b + c is the
    midpoint of c and its float32 neighbour towards zero, and 2^(t-46) of the exact sum is lost in it."""
    out = []
    for tt in range(-30, 31, 3):
        for k in (1, 2, 5, 4097, 2 ** 22 + 1):     # k >= 1: c is no power of two, its neighbours are equally far
            for sign in (1.0, -1.0):
                a = F(-sign * (1.0 + 2.0 ** -23))
                b = F(2.0 ** tt * (1.0 - 2.0 ** -23))
                c = F(sign * (2.0 ** (tt + 24) + k * 2.0 ** (tt + 1)))
                out.append((a, b, c, sign))
    return out


def test_fma_ties_follow_the_residual():
    """Triples whose float64 sum is a float32 midpoint with a residual of either sign: the twice-rounded sum breaks the tie to
    even, the exact fma by the residual; they differ wherever the even neighbour is the wrong one."""
    tri = _tie_triples()
    a, b, c = (np.array([x[i] for x in tri], dtype=F) for i in range(3))
    signs = set()
    for x, y, z, sign in tri:
        s64 = float(x) * float(y) + float(z)
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.nextafter(z, F(0.0))
        assert Fraction(s64) == (Fraction(float(z)) + Fraction(float(lo))) / 2        # a float32 midpoint
        assert exact != Fraction(s64)                                                 # with a non-zero residual
        assert (exact > Fraction(s64)) == (sign > 0)
        signs.add(exact > Fraction(s64))
    assert signs == {True, False}
    got = A.fma_f32(a, b, c)
    want = np.array([_exact(x, y, z) for x, y, z, _ in tri], dtype=F)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits(c))                # the residual always points back to c here
    twice = A.fma_f32_twice_rounded(a, b, c)
    wrong = _bits(twice) != _bits(want)
    assert wrong.any() and not wrong.all()                      # odd c: ties-to-even leaves it; even c: it agrees
    assert all(bool(w) == bool(int(_bits(z)) & 1) for w, (_, _, z, _) in zip(wrong, tri))


def test_fma_without_a_residual_rounds_ties_to_even():
    c = np.array([1.0, 1.0 + 2.0 ** -23], dtype=F)
    got = A.fma_f32(np.full(2, 2.0 ** -12, dtype=F), np.full(2, 2.0 ** -12, dtype=F), c)     # + 2^-24: exactly half an ulp
    assert np.array_equal(_bits(got), _bits(np.array([1.0, 1.0 + 2.0 ** -22], dtype=F)))


# -------------------------------------------------------------------------------------------------------------- constants
def _decimal_consts(lr, beta1, beta2, eps, step):
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    b1, b2 = D(beta1), D(beta2)                     # the doubles' exact values
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return [float(x) for x in (b1, b2, 1 - b1, 1 - b2, D(lr) / bc1, bc2.sqrt(), D(eps))]


@pytest.mark.parametrize("step", A.STEPS)
@pytest.mark.parametrize("hyper", A.HYPERS)
def test_constants_match_decimal_arithmetic(hyper, step):
    """The header's formulas in 60-digit decimal arithmetic from the same doubles, rounded to float32: equal to the double chain
    (pow, subtract, divide or sqrt, each within an ulp of float64) rounded to float32, for every set and step of the tables."""
    c = A.constants(*hyper, step)
    want = _decimal_consts(*hyper, step)
    assert all(type(x) is F for x in c)
    for name, got, w in zip(c._fields, c, want):
        assert got == F(w), (name, got, F(w))
    if step == 1:
        lr, beta1, beta2, _ = hyper
        assert c.step_size == F(lr / (1.0 - beta1)) and c.bc2_sqrt == F(math.sqrt(1.0 - beta2))


# ----------------------------------------------------------------------------------------- the optimizer the project states
def test_seven_step_trajectory_matches_float32_torch_adam():
    """test_adam_matches_torch_optim with `update` in the kernel's place, at its bars."""
    n, d = 257, 64
    g = t.Generator().manual_seed(2)
    p_ref = t.nn.Parameter(t.randn(n, d, generator=g) * 0.1)
    opt = t.optim.Adam([p_ref], lr=1e-3)
    p = p_ref.detach().clone().numpy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    worst = 0.0
    for step in range(1, 8):
        grad = t.randn(n, d, generator=g) * (10.0 ** -(step % 4))
        grad[step::7] = 0.0
        p_ref.grad = grad.clone()
        opt.step()
        p, m, v = A.update(p, grad.numpy(), m, v, A.constants(1e-3, 0.9, 0.999, 1e-8, step))
        worst = max(worst, A.bar_fraction(p, p_ref.detach().numpy(), "p"))
        assert t.allclose(t.from_numpy(p), p_ref.detach(), atol=2e-7, rtol=1e-6), step
    st = opt.state[p_ref]
    fr = dict(p=worst, m=A.bar_fraction(m, st["exp_avg"].numpy(), "m"), v=A.bar_fraction(v, st["exp_avg_sq"].numpy(), "v"))
    _report("seven steps vs float32 torch.optim.Adam", fr)
    assert t.allclose(t.from_numpy(m), st["exp_avg"], atol=1e-8, rtol=1e-5)
    assert t.allclose(t.from_numpy(v), st["exp_avg_sq"], atol=1e-12, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------ row copies
def test_row_copy_references_invert_each_other():
    rng = np.random.default_rng(9)
    rows = rng.permutation(A.ROW_COPY_TABLE)[:A.ROW_COPY_N] + 17
    src = rng.standard_normal((A.ROW_COPY_N, 8)).astype(F)
    for name, (begin, n) in A.ROW_COPY_WINDOWS.items():
        lo, hi = A.window(A.ROW_COPY_N, begin, n)
        table = np.full((A.ROW_COPY_TABLE, 8), np.nan, dtype=F)
        A.scatter_rows_ref(table, src, rows, 17, begin, n)
        assert int((~np.isnan(table[:, 0])).sum()) == hi - lo, name
        back = np.full_like(src, np.nan)
        A.gather_rows_ref(back, table, rows, 17, begin, n)
        assert np.array_equal(back[lo:hi], src[lo:hi]) and np.isnan(back[:lo]).all() and np.isnan(back[hi:]).all()
        acc = src.copy()
        A.gather_rows_ref(acc, table, rows, 17, begin, n, accumulate=True, scale=0.5)
        assert np.array_equal(acc[lo:hi], (src[lo:hi] + src[lo:hi]) * F(0.5)) and np.array_equal(acc[:lo], src[:lo])
    assert {A.window(A.ROW_COPY_N, *w) for w in A.ROW_COPY_WINDOWS.values()} == {(0, 150), (37, 101), (60, 60), (0, 0), (45, 150), (0, 77)}


# ------------------------------------------------------------------------------------------------------------ case tables
def _dispatch(entries):
    """The rule in the header at mi_adam_multi_f32: empty tensors are skipped; a tensor of at least 65536 elements whose count
    is a multiple of 4 and whose four pointers are 16-byte aligned goes to the dense kernel; every other one is appended to
    a table that is launched when it holds 48 tensors, and once more at the end if it holds any."""
    out, in_table, launches = [], 0, 0
    for e in entries:
        aligned = all((4 * e["mis"][k]) % 16 == 0 for k in "pgmv")
        if e["n"] == 0:
            out.append(("skip", None))
        elif e["n"] >= 65536 and e["n"] % 4 == 0 and aligned:
            out.append(("dense", None))
        else:
            out.append(("table", launches))
            in_table += 1
            if in_table == 48:
                in_table, launches = 0, launches + 1
    return out, launches + (1 if in_table else 0)


def test_multi_lists_say_what_the_dispatcher_does():
    for name, entries in A.MULTI_LISTS.items():
        got, launches = _dispatch(entries)
        assert got == [(e["path"], e["flush"]) for e in entries], name
        assert launches == {"sizes": 1, "flush": 2}[name]
    sizes = A.MULTI_LISTS["sizes"]
    assert [e["n"] for e in sizes] == [0, 1, 3, 255, 256, 257, 16383, 16384, 16385, 65535, 65536, 65540, 65538, 65536]
    assert [e["path"] for e in sizes[-4:]] == ["dense", "table", "table", "table"]
    assert -(-65540 // (A.MULTI_GRID_X * A.ADAM_BLOCK)) == 5                         # grid-stride passes of the longest
    flush = A.MULTI_LISTS["flush"]
    assert sum(e["path"] == "table" for e in flush) == 53 and [e["flush"] for e in flush if e["path"] == "table"] == [0] * 48 + [1] * 5
    assert flush[26]["path"] == "dense" and 0 < 26 < len(flush) - 1


def test_dense_cases_reach_every_lane_layout():
    lpr = {d: A.lanes_per_row(d) for d in A.DENSE_WIDTHS}
    assert lpr == {4: 1, 12: 4, 64: 16, 200: 64, 260: 128, 1024: 256, 1028: 256, 2052: 256}
    assert {d: -(-(d // 4) // lpr[d]) for d in A.DENSE_WIDTHS} == {4: 1, 12: 1, 64: 1, 200: 1, 260: 1, 1024: 1, 1028: 2, 2052: 3}
    for d in A.DENSE_WIDTHS:
        rpb = A.ADAM_BLOCK // lpr[d]
        ns = {c["n_rows"] for c in A.DENSE_CASES if c["d"] == d}
        assert {1, rpb + 1, 257} <= ns and (rpb == 1 or rpb - 1 in ns)
        for n in ns:
            assert {(c["reg_w"], c["strided"]) for c in A.DENSE_CASES if c["d"] == d and c["n_rows"] == n} == {
                (False, False), (False, True), (True, False), (True, True)}
    c = A.GRID_CAP_CASE   # one lane per row: the capped grid's first pass takes 256 * 32 * 256 rows, the second the other 300
    assert A.lanes_per_row(c["d"]) == 1 and c["n_rows"] - A.ADAM_GRID_CAP * A.ADAM_BLOCK == 300
    assert len(A.RANKER_SIZES) == A.MULTI_MAX_PARAMS and sum(n > A.MULTI_GRID_X * A.ADAM_BLOCK for n in A.RANKER_SIZES) == 2
