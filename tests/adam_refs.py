"""Host references and case tables for the dense Adam update and the row-copy kernels — written from csrc/common.hpp
(mi_adam_consts, mi_adam_update4), the header text at mi_adam_multi_f32 and the docstrings of ops.gather_rows / ops.scatter_rows.

Shared by tests/test_adam_refs_cpu.py (the references against exact rational arithmetic, a float64 torch.optim.Adam and the
float32 torch.optim.Adam) and tests/test_gpu_adam.py (every launch form of the kernels against the references, bit for bit).

Every operation of mi_adam_update4 is one correctly rounded IEEE float32 operation, so `update` restates it exactly: NumPy's
float32 +, -, *, / and sqrt are correctly rounded and never contracted, and the one fused multiply-add is computed exactly
(fma_f32).  The only tolerances here are the three bars of test_adam_matches_torch_optim (BARS), used against the float64 twin.
"""
import collections
import math

import numpy as np
import torch as t

F = np.float32

# (atol, rtol) of test_adam_matches_torch_optim, for p, exp_avg and exp_avg_sq
BARS = {"p": (2e-7, 1e-6), "m": (1e-8, 1e-5), "v": (1e-12, 1e-5)}

HYPERS = ((1e-3, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-6), (3e-4, 0.0, 0.99, 1e-10))   # lr, beta1, beta2, eps
STEPS = (1, 2, 7, 1000, 100000)

Consts = collections.namedtuple("Consts", "b1 b2 omb1 omb2 step_size bc2_sqrt eps")


def constants(lr, beta1, beta2, eps, step):
    """mi_adam_consts: the bias corrections in double, each of the seven scalars rounded once to float32."""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return Consts(F(beta1), F(beta2), F(1.0 - beta1), F(1.0 - beta2), F(lr / bc1), F(math.sqrt(bc2)), F(eps))


# ------------------------------------------------------------------------------------------------------------ exact fma
def fma_f32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, elementwise on float32 arrays.

    a * b is exact in float64 (24 + 24 significand bits).  s = fl64(ab + c) with its error-free residual e (Knuth's two-sum).
    Rounding to float64 is monotone and every float32 midpoint is a float64, so rounding s to float32 differs from rounding
    the exact sum only where s IS a midpoint between two neighbouring float32 values and e != 0: there the sign of e decides."""
    a, b, c = (np.asarray(x, dtype=F) for x in (a, b, c))
    prod = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    s = prod + cd
    bb = s - prod
    e = (prod - (s - bb)) + (cd - bb)
    with np.errstate(over="ignore"):
        r = s.astype(F)                                       # ties to even: right when e == 0
        rd = r.astype(np.float64)
        toward = np.where(s > rd, F(np.inf), F(-np.inf)).astype(F)
        other = np.nextafter(r, toward)                       # the float32 neighbour on s's side of r
        tie = (rd != s) & np.isfinite(r) & np.isfinite(other) & ((rd + other.astype(np.float64)) * 0.5 == s) & (e != 0.0)
    lo, hi = np.minimum(r, other), np.maximum(r, other)
    return np.where(tie, np.where(e > 0.0, hi, lo), r).astype(F)


def fma_f32_twice_rounded(a, b, c):
    """What fma_f32 must NOT be: the float64 sum rounded to float32 (two roundings).  Kept for the tests that tell them apart."""
    a, b, c = (np.asarray(x, dtype=F) for x in (a, b, c))
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


# ---------------------------------------------------------------------------------------------------------------- update
def update(p, g, m, v, consts, reg_w=None, g_scale=1.0):
    """mi_adam_update4 on float32 arrays of one shape ([n] or [n, d]); returns (p', m', v'), the inputs are not written.
    reg_w float32 [n]: the per-row L2 weight of a [n, d] table.  g_scale: adam_multi_kernel's gradient scale (a float)."""
    p, g, m, v = (np.asarray(x) for x in (p, g, m, v))
    assert p.dtype == g.dtype == m.dtype == v.dtype == F and p.shape == g.shape == m.shape == v.shape
    c = consts
    assert all(type(x) is F for x in c)
    if F(g_scale) != F(1.0):
        g = g * F(g_scale)
    if reg_w is not None:
        w = np.asarray(reg_w)
        assert w.dtype == F and w.shape == p.shape[:1] and p.ndim == 2
        g = fma_f32(np.broadcast_to(w[:, None], p.shape), p, g)
    m1 = c.b1 * m + c.omb1 * g
    v1 = c.b2 * v + (c.omb2 * g) * g
    p1 = p - c.step_size * (m1 / (np.sqrt(v1) / c.bc2_sqrt + c.eps))
    assert p1.dtype == m1.dtype == v1.dtype == F
    return p1, m1, v1


def twin_f64(p, g, m, v, hyper, step, reg_w=None, g_scale=1.0):
    """One step of torch.optim.Adam on float64 copies of the float32 state (step, exp_avg, exp_avg_sq set by hand): the
    independent reference.  Returns float64 arrays (p', m', v')."""
    lr, beta1, beta2, eps = hyper
    pd = t.from_numpy(np.asarray(p, dtype=np.float64).copy()).requires_grad_(True)
    gd = t.from_numpy(np.asarray(g, dtype=np.float64).copy()) * float(F(g_scale))
    if reg_w is not None:
        gd = gd + t.from_numpy(np.asarray(reg_w, dtype=np.float64))[:, None] * pd.detach()
    opt = t.optim.Adam([pd], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    opt.state[pd] = {"step": t.tensor(float(step - 1)), "exp_avg": t.from_numpy(np.asarray(m, dtype=np.float64).copy()),
                     "exp_avg_sq": t.from_numpy(np.asarray(v, dtype=np.float64).copy())}
    pd.grad = gd
    opt.step()
    st = opt.state[pd]
    assert float(st["step"]) == float(step)
    return pd.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def bar_fraction(got, ref, name):
    """max over elements of |got - ref| / (atol + rtol * |ref|) for BARS[name]: <= 1 is what allclose accepts."""
    atol, rtol = BARS[name]
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def state(shape, seed, zero_moments=False):
    """(p, g, m, v) float32: p ~ 0.1, |g| from 1e-3 to 1 by position, m ~ 0.01, v in [0, 1e-3).  Every seventh gradient entry is
    exactly zero, and every third of those has zero moments as well (such a parameter must keep its bits)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    idx = np.arange(n)
    p = (rng.standard_normal(n) * 0.1).astype(F)
    g = (rng.standard_normal(n) * 10.0 ** -(idx % 4)).astype(F)
    m = (rng.standard_normal(n) * 0.01).astype(F)
    v = (rng.random(n) * 1e-3).astype(F)
    if zero_moments:
        m[:], v[:] = 0.0, 0.0
    g[idx % 7 == 3] = 0.0
    still = idx % 21 == 3
    m[still], v[still] = 0.0, 0.0
    return tuple(x.reshape(shape) for x in (p, g, m, v))


def still_mask(shape):
    """The entries of state(shape, ...) with zero gradient and zero moments."""
    return (np.arange(int(np.prod(shape))) % 21 == 3).reshape(shape)


# ------------------------------------------------------------------------------------------------------------- row copies
def window(n_max, begin, n):
    """[begin, n) as the kernels read it: a missing begin is 0, a missing n is n_max; clipped to n_max."""
    lo = 0 if begin is None else begin
    hi = n_max if n is None else min(n, n_max)
    return lo, max(hi, lo)


def gather_rows_ref(dst, src, rows, row_offset=0, begin=None, n=None, accumulate=False, scale=1.0):
    """In place: dst[i] = scale * ((accumulate ? dst[i] : 0) + src[rows[i] - row_offset]) for i in [begin, n); the multiply only
    when float32(scale) != 1."""
    assert dst.dtype == src.dtype == F
    lo, hi = window(len(rows), begin, n)
    for i in range(lo, hi):
        x = src[int(rows[i]) - row_offset]
        if accumulate:
            x = dst[i] + x
        if F(scale) != F(1.0):
            x = x * F(scale)
        dst[i] = x


def scatter_rows_ref(dst, src, rows, row_offset=0, begin=None, n=None):
    """In place: dst[rows[i] - row_offset] = src[i] for i in [begin, n) (rows distinct)."""
    assert dst.dtype == src.dtype == F
    lo, hi = window(len(rows), begin, n)
    for i in range(lo, hi):
        dst[int(rows[i]) - row_offset] = src[i]


# ------------------------------------------------------------------------------------------------------------ case tables
ADAM_BLOCK = 256              # threads of adam_kernel's block
ADAM_GRID_CAP = 256 * 32      # blocks of mi_adam_dense_f32's grid, the rest by the grid-stride loop
DENSE_WIDTHS = (4, 12, 64, 200, 260, 1024, 1028, 2052)


def lanes_per_row(d):
    """adam_kernel: the smallest power of two >= d / 4, capped at the block."""
    lpr = 1
    while lpr < d // 4 and lpr < ADAM_BLOCK:
        lpr <<= 1
    return lpr


def _dense_cases():
    out = []
    for d in DENSE_WIDTHS:
        rpb = ADAM_BLOCK // lanes_per_row(d)             # rows one block takes per pass
        for n_rows in sorted({1, max(rpb - 1, 1), rpb + 1, 257}):
            for reg_w in (False, True):
                for strided in (False, True):
                    out.append(dict(d=d, n_rows=n_rows, reg_w=reg_w, strided=strided))
    return out


DENSE_CASES = _dense_cases()
DENSE_PAD_P, DENSE_PAD_G = 4, 8                         # strided cases: ldp = d + 4, ldgr = d + 8
GRID_CAP_CASE = dict(d=4, n_rows=ADAM_GRID_CAP * ADAM_BLOCK + 300, reg_w=True, strided=False)
HYPER_SHAPE = (130, 200)

MULTI_DENSE_MIN = 65536       # mi_adam_multi_f32: at least this many elements, % 4 == 0, four aligned pointers -> dense kernel
MULTI_MAX_PARAMS = 48         # MI_RANKER_MAX_PARAMS: tensors per table launch
MULTI_GRID_X = 64             # blocks in x of a table launch


def _entry(n, path, flush=None, **misaligned):
    """One tensor of a list: n elements; the operands named in `misaligned` start that many floats past a 16-byte boundary.
    path / flush: what the dispatcher must do with it ("skip", "dense", or "table" in the flush-th table launch)."""
    return dict(n=n, path=path, flush=flush, mis={k: misaligned.get(k, 0) for k in "pgmv"})


def _flush_list():
    out, tabled = [], 0
    for i in range(54):
        if i == 26:
            out.append(_entry(65544, "dense"))
            continue
        out.append(_entry(1 + (i * 37) % 300, "table", tabled // MULTI_MAX_PARAMS))
        tabled += 1
    return out


MULTI_LISTS = {
    "sizes": [_entry(0, "skip")] + [_entry(n, "table", 0) for n in (1, 3, 255, 256, 257, 16383, 16384, 16385, 65535)] + [
        _entry(65536, "dense"),
        _entry(65540, "table", 0, p=1),      # large but p misaligned: ceil(65540 / (64 * 256)) = 5 grid passes
        _entry(65538, "table", 0),           # large and aligned, not a multiple of 4
        _entry(65536, "table", 0, g=1),      # only the gradient misaligned
    ],
    "flush": _flush_list(),                  # 53 table tensors: 48 in the first launch, 5 in the second; one dense between
}

RANKER_SIZES = tuple([1, 3, 255, 256, 257, 16385, 20000] + [2 + (i * 53) % 400 for i in range(41)])   # 48; two take > 1 pass
RANKER_GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0)

ROW_COPY_WIDTHS = (4, 36, 256, 260, 512)                 # d / 4 > 64 for 260 and 512: the lane loop's second trip
ROW_COPY_CASES = [dict(d=d, strided=s, row_offset=o) for d in ROW_COPY_WIDTHS for s in (False, True) for o in (0, 17)]
ROW_COPY_N, ROW_COPY_TABLE = 150, 170                    # rows copied (38 blocks of 4 wavefronts), rows of the table
ROW_COPY_WINDOWS = {                                     # name -> (begin, n); None = the pointer is not given
    "full": (None, None), "interior": (37, 101), "empty": (60, 60), "n=0": (None, 0), "begin only": (45, None),
    "n only": (None, 77),
}
ROW_COPY_MODES = [(a, s) for a in (False, True) for s in (1.0, 0.5)]   # accumulate, scale
