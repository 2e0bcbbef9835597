"""The bf16-layer rule of include/laplace_hip.h ("bf16 layer tables") restated in numpy / torch, the float64 reference of its
product with the quantities the derived bounds need, and the inputs both test files use.  Nothing here is shared with the code
under test: f32 fma chains are adam_refs.fma_f32 (one rounding), rn is tensor.to(torch.bfloat16).

    X_0 = rn(E0);  acc_k = A float(X_{k-1}) in f32 fma chains;  X_k = rn(acc_k), k < K;
    final = c * (E0 + float(X_1) + ... + float(X_{K-1}) + acc_K), added in this order.
"""
import numpy as np
import torch as t

from adam_refs import fma_f32

F = np.float32
U32 = 2.0 ** -24   # unit roundoff of f32
U16 = 2.0 ** -8    # the bound the tests grant a bf16 rounding (8 significand bits)

N_ROWS, N_COLS = 333, 257
WIDTHS = (8, 24, 64, 128, 256)
PLANS = (None, (8, 0), (8, 64))   # (chunk, band) of ops.build_spmm_plan; None = no plan


def rn(x):
    """f32 array -> the f32 values of its bf16 rounding (round to nearest even)."""
    return t.from_numpy(np.ascontiguousarray(x, dtype=F)).to(t.bfloat16).float().numpy()


def bf16_tensor(x):
    """f32 array whose values are bf16-representable -> torch.bfloat16 tensor (exact)."""
    return t.from_numpy(np.ascontiguousarray(x, dtype=F)).to(t.bfloat16)


def adjacency(seed=0):
    """(rowptr int32 [334], col int32, val f32): 333 x 257, columns ascending within a row.  The first rows have 0, 1, 7, 8, 9,
    100 and all 257 entries (every class against chunk = 8: empty, short, chunk - 1, chunk, chunk + 1, split, split across every
    band of 64 columns); the others 0..20 entries, the last row empty again."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 7, 8, 9, 100, N_COLS] + [int(x) for x in rng.integers(0, 21, size=N_ROWS - 8)] + [0]
    cols = [np.sort(rng.choice(N_COLS, size=n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.zeros(N_ROWS + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(lens)
    col = np.concatenate(cols).astype(np.int32)
    val = rng.standard_normal(col.size).astype(F)
    return rowptr, col, val


def operand(d, seed=1):
    """bf16-representable f32 [257, d], and an f32 addend [333, d]."""
    rng = np.random.default_rng(seed + d)
    return rn(rng.standard_normal((N_COLS, d)).astype(F)), rng.standard_normal((N_ROWS, d)).astype(F)


def row_list():
    """Repeats, rows of every class, the empty rows; (list int32, device count < its length)."""
    rows = np.array([6, 0, 5, 3, 6, 1, 200, 4, 2, 332, 17, 5, 100, 6, 0, 250, 33], dtype=np.int32)
    return rows, 13


def exact_case(d):
    """val in {0.5, 1, 2} and small integer X: every f32 sum is exact (|sum| <= 257 * 2 * 8 < 2^24)."""
    rowptr, col, _ = adjacency()
    rng = np.random.default_rng(7)
    val = rng.choice(np.array([0.5, 1.0, 2.0], dtype=F), size=col.size)
    x = rng.integers(-8, 9, size=(N_COLS, d)).astype(F)
    return rowptr, col, val, x


# ---------------------------------------------------------------------------------------------- the float64 reference
def spmm_f64(rowptr, col, val, x, rows=None):
    """(exact, absum, n) per output element / row: exact = sum val * x in float64, absum = sum |val * x|, n = entries."""
    rows = np.arange(len(rowptr) - 1) if rows is None else np.asarray(rows)
    d = x.shape[1]
    exact = np.zeros((len(rows), d))
    absum = np.zeros((len(rows), d))
    n = np.zeros(len(rows), dtype=np.int64)
    xd, vd = x.astype(np.float64), val.astype(np.float64)
    for i, r in enumerate(rows):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        prod = vd[b:e, None] * xd[col[b:e]]
        exact[i], absum[i], n[i] = prod.sum(0), np.abs(prod).sum(0), e - b
    return exact, absum, n


def chain_error(n, absum):
    """E = n u32 / (1 - n u32) * absum: any fixed order of f32 fma chains and partial sums over n entries."""
    n = np.asarray(n, dtype=np.float64)[:, None]
    return n * U32 / (1.0 - n * U32) * absum


def bound_s(n, absum, exact, addend, scale):
    """f32 S without Y: |scale| (E + 2 u32 |addend + exact|); absum counts |addend| too."""
    a = 0.0 if addend is None else addend.astype(np.float64)
    return abs(scale) * (chain_error(n, absum + np.abs(a)) + 2.0 * U32 * np.abs(a + exact))


def bound_y(n, absum, exact):
    """A stored Y: u16 (|exact| + E) + E."""
    e = chain_error(n, absum)
    return U16 * (np.abs(exact) + e) + e


def bound_s_with_y(n, absum, exact, addend, scale):
    """S beside Y: the Y bound times |scale|, plus the f32 terms."""
    return abs(scale) * bound_y(n, absum, exact) + bound_s(n, absum, exact, addend, scale)


# ---------------------------------------------------------------------------------------------------------- the mirror
def spmm_mirror(rowptr, col, val, x, chunk=None, rows=None):
    """acc f32 [rows, d]: a row of at most `chunk` entries (or any row, chunk None) is one fma chain in list order from 0; a
    longer row is one such chain per consecutive piece of `chunk` entries, the partial rows added in piece order."""
    rows = np.arange(len(rowptr) - 1) if rows is None else np.asarray(rows)
    d = x.shape[1]
    out = np.zeros((len(rows), d), dtype=F)

    def chain(b, e):
        acc = np.zeros(d, dtype=F)
        for p in range(b, e):
            acc = fma_f32(np.full(d, val[p], dtype=F), x[col[p]], acc)
        return acc
    for i, r in enumerate(rows):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if chunk is None or e - b <= chunk:
            out[i] = chain(b, e)
        else:
            tot = np.zeros(d, dtype=F)
            for pb in range(b, e, chunk):
                tot = (tot + chain(pb, min(e, pb + chunk))).astype(F)
            out[i] = tot
    return out


def epilogue_mirror(acc, want_y, addend, scale):
    """(Y as f32 values or None, S): Y = rn(acc); S = scale * (addend + (Y ? float(Y) : acc)) in f32, one rounding each."""
    y = rn(acc) if want_y else None
    v = y if want_y else acc
    a = np.zeros_like(acc) if addend is None else addend.astype(F)
    s = (F(scale) * (a + v).astype(F)).astype(F)
    return y, s


def propagate_mirror(rowptr, col, val, e0, K, chunk=None):
    """(final f32, [X_0 .. X_{K-1}] as f32 values, the sequence of partial layer sums): the rule, layer by layer."""
    e0 = np.ascontiguousarray(e0, dtype=F)
    if K == 0:
        return e0.copy(), [], [e0.copy()]
    c = F(1.0 / (K + 1))
    xs = [rn(e0)]
    run = e0.copy()
    sums = [run.copy()]
    for k in range(1, K):
        xk = rn(spmm_mirror(rowptr, col, val, xs[-1], chunk))
        run = (run + xk).astype(F)
        sums.append(run.copy())
        xs.append(xk)
    acc = spmm_mirror(rowptr, col, val, xs[-1], chunk)
    run = (run + acc).astype(F)
    sums.append(run.copy())
    return (c * run).astype(F), xs, sums
