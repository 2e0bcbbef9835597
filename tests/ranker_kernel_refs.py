"""Float64 references, error bounds and test data for the ranker's element kernels (csrc/norm.hip, csrc/sage.hip) — written from
include/laplace_hip.h and torch's definitions of BatchNorm1d, BCEWithLogitsLoss, Embedding(max_norm) and scatter-max.

Shared by tests/test_ranker_kernel_refs_cpu.py (the bounds admit a float32 evaluation of the same formulas and refuse a worse
one) and tests/test_gpu_ranker_kernels.py (the kernels against the references).

Every bound is a count of float32 roundings times the magnitude of what was rounded, U = 2^-24 (the unit roundoff of a correctly
rounded float32 operation) per rounding.  Sums the kernels keep in double contribute n * 2^-52 of the
summed magnitudes, which is written out where it matters.  No constant here was fitted to a kernel's output.
"""
import numpy as np
import torch as t

U = 2.0 ** -24
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ batch-norm
BN_WIDTHS = (4, 8, 16, 32, 128, 256, 512, 12, 68)   # 16-byte walk: powers of two up to 256; 12, 68: scalar walk + vec4 apply
BN_LAYOUT_WIDTHS = (4, 64, 256)
BN_ROWS = (2, 777)
BN_LAYOUTS = ("contiguous", "ld+4", "ld+1", "offset1")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_case(n, c, seed=0):
    """x [n, c], gamma, beta, dy, running_mean, running_var (float32, CPU).  Column j has mean ~100 and spread 0.1 where
    j % 4 == 1 (the columns that need the double sums), else spread 2 around a mean of a few units.  gamma has both signs.
    beta is given the sign of -mean * gamma: with it |mean * invstd * gamma| <= |x * invstd * gamma| + |y| holds for every
    element, which is what makes the issue's bound for y a derived one (bn_y_worst_case below)."""
    g = t.Generator().manual_seed(1000 * c + n + seed)
    x = t.randn(n, c, generator=g) * 2.0 + 3.0 * t.randn(1, c, generator=g)
    hard = t.arange(c) % 4 == 1
    x[:, hard] = 100.0 + 0.1 * t.randn(n, int(hard.sum()), generator=g)
    gamma = (t.rand(c, generator=g) + 0.5) * t.where(t.rand(c, generator=g) < 0.3, -1.0, 1.0)
    beta = t.randn(c, generator=g).abs() * -t.sign(x.double().mean(0) * gamma).float()
    dy = t.randn(n, c, generator=g)
    rm, rv = t.randn(c, generator=g), t.rand(c, generator=g) + 0.5
    return x, gamma, beta, dy, rm, rv


def bn_fwd_ref(x, gamma, beta, rm, rv, eps=BN_EPS, momentum=BN_MOMENTUM):
    """Training-mode BatchNorm1d in float64 from float32 inputs: dict of y, mean, invstd, running_mean, running_var (the
    running variance takes the unbiased batch variance), var and ex2 = E[x^2] for the bounds."""
    xd, n = x.double(), x.shape[0]
    m = xd.mean(0)
    var = ((xd - m) ** 2).mean(0)
    invstd = 1.0 / t.sqrt(var + eps)
    y = (xd - m) * invstd * gamma.double() + beta.double()
    unb = var * (n / (n - 1.0)) if n > 1 else var
    return dict(y=y, mean=m, invstd=invstd, var=var, ex2=(xd * xd).mean(0), unb=unb,
                running_mean=(1.0 - momentum) * rm.double() + momentum * m,
                running_var=(1.0 - momentum) * rv.double() + momentum * unb)


def bn_y_bound(x, ref, gamma):
    """8 U (|x| invstd |gamma| + |y_ref|), elementwise."""
    return 8.0 * U * (x.double().abs() * ref["invstd"] * gamma.double().abs() + ref["y"].abs())


def bn_y_worst_case(x, ref, gamma, beta):
    """Worst case of y = fma(x, scale, shift) with scale = fl(invstd * gamma), shift = fl(beta - fl(fl(mean * invstd) * gamma)),
    mean and invstd rounded from double.  A = |x invstd gamma|, M = |mean invstd gamma|, B = |beta|, Y = |y|:
        scale carries 2 roundings (invstd, the product)                  -> 2 U A
        shift carries 4 on M (mean, invstd, two products) and its own    -> 4 U M + U (M + B)
        the fma rounds once                                              -> U Y
    With beta of the sign of -mean * gamma, |y| >= |A - (M + B)|, and 2 A + 5 M + B + Y <= 8 (A + Y) follows in both cases
    (A <= M + B: 6 A + 7 Y >= 7 (M + B) - A >= 5 M + B;  A > M + B: 6 A > 5 M + B).  The CPU tests assert it, with the double sums'
    share, for every case the GPU tests run."""
    n = x.shape[0]
    A = x.double().abs() * ref["invstd"] * gamma.double().abs()
    M = (ref["mean"] * ref["invstd"] * gamma.double()).abs()
    sums = 0.5 * bn_var_abs_err(n, ref) / (ref["var"] + BN_EPS) * (ref["y"] - beta.double()).abs()   # invstd from the double sums
    return U * (2 * A + 4 * M + (M + beta.double().abs()) + ref["y"].abs()) + sums


def bn_var_abs_err(n, ref):
    """Absolute error of the variance from sums kept in double as E[x^2] - mean^2: each of the n adds rounds at 2^-53 of a partial
    sum <= n E[x^2]; the same for the mean, which enters squared (twice): 3 n 2^-53 E[x^2]."""
    return 3.0 * n * 2.0 ** -53 * ref["ex2"]


def bn_stat_bounds(n, ref, rm, rv, momentum=BN_MOMENTUM, eps=BN_EPS):
    """Bounds for save_mean, save_invstd, running_mean, running_var.  mean, invstd: one rounding to float32 plus the double
    sums' own error (invstd moves by half the relative error of var + eps).  Running statistics: fl(1 - momentum), fl(momentum),
    two products and the sum — 3 roundings on each addend — on top of the new statistic's own error."""
    var_err = bn_var_abs_err(n, ref)
    mean_b = U * ref["mean"].abs() + n * 2.0 ** -52 * ref["ex2"].sqrt()
    unb_err = var_err * (n / (n - 1.0) if n > 1 else 1.0) + U * ref["unb"]             # (float)unb
    return dict(mean=mean_b, invstd=ref["invstd"] * (U + 0.5 * var_err / (ref["var"] + eps)),
                running_mean=3 * U * (((1 - momentum) * rm.double()).abs() + (momentum * ref["mean"]).abs()) + momentum * mean_b,
                running_var=3 * U * (((1 - momentum) * rv.double()).abs() + momentum * ref["unb"]) + momentum * unb_err)


def bn_bwd_ref(x, dy, gamma, mean, invstd):
    """Backward of training-mode batch-norm in float64, from the float32 x, dy, gamma and the float32 mean / invstd the forward
    saved: dict of dx, dgamma, dbeta and the bounds.
        xhat = fl(fl(x - mean) invstd): 2 roundings.  dbeta = sum dy and dgamma = sum dy xhat are summed in double and
        rounded once: dbeta <= U |dbeta| + n 2^-52 sum|dy|;  dgamma <= 3 U sum|dy xhat| (xhat's two, the store).
        dx = G (dy - a - xhat b), G = fl(gamma invstd), a = fl(dbeta / n), b = fl(dgamma / n).  With T = |dy| + |a| + |xhat b|:
        a: 1 rounding, xhat b: xhat's 2 + b's 1 + the product = 4, two subtractions and G's two roundings on at most T each = 4,
        <= 8 U |G| T in all; b also carries dgamma's summed error 3 U mean|dy xhat|, scaled by |xhat|."""
    xd, dyd, n = x.double(), dy.double(), x.shape[0]
    xhat = (xd - mean.double()) * invstd.double()
    dbeta, dgamma = dyd.sum(0), (dyd * xhat).sum(0)
    G = gamma.double() * invstd.double()
    a, b = dbeta / n, dgamma / n
    mass = (dyd * xhat).abs().sum(0)
    T = dyd.abs() + a.abs() + (xhat * b).abs()
    return dict(dx=G * (dyd - a - xhat * b), dgamma=dgamma, dbeta=dbeta,
                dbeta_bound=U * dbeta.abs() + n * 2.0 ** -52 * dyd.abs().sum(0),
                dgamma_bound=3 * U * mass + n * 2.0 ** -52 * mass,
                dx_bound=U * G.abs() * (8 * T + 3 * xhat.abs() * mass / n))


def bn_emulate(x, gamma, beta, eps=BN_EPS, double_sums=True):
    """NumPy emulations of the forward.  double_sums=True: the kernel's arithmetic (sums of x and x^2 in double, mean and invstd
    rounded to float32, y = fl(x * scale + shift) — NumPy has no fma, the extra rounding is inside the bound).  False: the
    deliberately worse one, E[x^2] - mean^2 in float32 running sums.  Returns (y, mean, invstd) as float32."""
    xn, gn, bn_ = x.numpy(), gamma.numpy(), beta.numpy()
    n = xn.shape[0]
    if double_sums:
        m = xn.astype(np.float64).sum(0) / n
        var = np.maximum((xn.astype(np.float64) ** 2).sum(0) / n - m * m, 0.0)
        mu, is_ = m.astype(F32), (1.0 / np.sqrt(var + eps)).astype(F32)
    else:
        sa, sb = np.zeros(xn.shape[1], F32), np.zeros(xn.shape[1], F32)
        for r in range(n):
            sa = sa + xn[r]
            sb = sb + xn[r] * xn[r]
        mu = sa / F32(n)
        var = np.maximum(sb / F32(n) - mu * mu, F32(0))
        is_ = F32(1) / np.sqrt(var + F32(eps))
    scale = is_ * gn
    shift = bn_ - mu * is_ * gn
    return t.from_numpy(xn * scale + shift), t.from_numpy(mu), t.from_numpy(is_)


def bn_bwd_emulate(x, dy, gamma, mean, invstd):
    """The backward kernel's arithmetic in NumPy float32 with double sums: (dx, dgamma, dbeta) as float32."""
    xn, gn, yn, mu, is_ = x.numpy(), gamma.numpy(), dy.numpy(), mean.numpy(), invstd.numpy()
    n = xn.shape[0]
    xh = (xn - mu) * is_
    sa, sb = yn.astype(np.float64).sum(0), (yn.astype(np.float64) * xh.astype(np.float64)).sum(0)
    a, b, G = (sa / n).astype(F32), (sb / n).astype(F32), gn * is_
    return t.from_numpy(G * (yn - a - xh * b)), t.from_numpy(sb.astype(F32)), t.from_numpy(sa.astype(F32))


# ------------------------------------------------------------------------------------------------------------------- BCE
BCE_SIZES = (1, 1023, 1024, 1025, 5000)
BCE_PLANTS = (100.0, -100.0, 88.0, -88.0, 20.0, -20.0, 0.0, -0.0, 1e-8, -1e-8)


def bce_case(n, seed=0):
    """logits = 4 randn with every planted value twice from index 1 on, once under label 0 and once under label 1 (n = 1 has
    room for the random draw only); labels 0 / 1 with a soft label in (0, 1) at every 97th of the other positions."""
    g = t.Generator().manual_seed(7 * n + seed)
    x = 4.0 * t.randn(n, generator=g)
    y = (t.rand(n, generator=g) < 0.4).float()
    soft = t.rand(n, generator=g) * 0.98 + 0.01
    y[50::97] = soft[50::97]
    k = len(BCE_PLANTS)
    if n >= 1 + 2 * k:
        x[1:1 + k] = t.tensor(BCE_PLANTS)
        x[1 + k:1 + 2 * k] = t.tensor(BCE_PLANTS)
        y[1:1 + k], y[1 + k:1 + 2 * k] = 0.0, 1.0
    return x, y


def bce_ref(x, y):
    """BCEWithLogitsLoss(mean) in float64 (torch's formulation) and its gradient: loss, dx, loss bound 4 U mean|term|, gradient
    bound 8 U / n."""
    xd, yd, n = x.double(), y.double(), x.numel()
    term = xd.clamp(min=0) - xd * yd + t.log1p(t.exp(-xd.abs()))
    return dict(loss=term.mean(), dx=(t.sigmoid(xd) - yd) / n, loss_bound=4 * U * term.abs().mean(), dx_bound=8 * U / n)


def bce_emulate(x, y, float_sum=False):
    """The formula in NumPy float32; the terms are summed in double (the kernel) or, float_sum=True, in one float32 running sum
    (the deliberately worse emulation).  Returns (loss, dx) as float32."""
    xn, yn = x.numpy(), y.numpy()
    n = xn.size
    with np.errstate(over="ignore"):
        term = np.maximum(xn, F32(0)) - xn * yn + np.log1p(np.exp(-np.abs(xn)))
        dx = (F32(1) / (F32(1) + np.exp(-xn)) - yn) * (F32(1) / F32(n))
    assert term.dtype == dx.dtype == F32
    if float_sum:
        loss = np.cumsum(term, dtype=F32)[-1] / F32(n)
    else:
        loss = F32(term.astype(np.float64).sum() / n)
    return float(loss), t.from_numpy(dx)


# ---------------------------------------------------------------------------------------------------------- embed_concat
EMBED_N, EMBED_ROWS = 101, 50
# (name, widths, per-table scale): rows of a width-w randn table have norm ~ sqrt(w) * scale
EMBED_CASES = (
    ("w64", [64], [1.0]), ("w64_small", [64], [0.01]), ("w65", [65], [1.0]), ("w128", [128], [0.01]), ("w200", [200], [1.0]),
    ("w4_w130", [4, 130], [0.02, 1.0]),
    ("twenty", [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1, 3, 96, 8, 40],
     [5.0, 0.02, 5.0, 0.02, 5.0, 0.02, 5.0, 0.02, 5.0, 0.02, 5.0, 0.02, 5.0, 0.02, 5.0, 5.0, 0.02, 1.0, 5.0, 0.01]),
)


def embed_case(name, seed=0):
    """tables (float32 [50, w]) and ids x [101, n_cols] of the named case."""
    _, widths, scales = next(c for c in EMBED_CASES if c[0] == name)
    g = t.Generator().manual_seed(seed + 31 * len(widths) + widths[-1])
    tables = [t.randn(EMBED_ROWS, w, generator=g) * s for w, s in zip(widths, scales)]
    x = t.randint(0, EMBED_ROWS, (EMBED_N, len(widths)), generator=g)
    return tables, x


def embed_ref(x, tables, max_norm):
    """cat_i Embedding_i(max_norm)(x[:, i]) in float64: the row where its norm <= max_norm, else row * max_norm / (norm + 1e-7).
    Returns (want, bound, near): bound = (dim / 2 + 4) U |want| (an fp32 sum of dim squares is within dim U relative, halved by
    the square root; then the add of 1e-7, the divide, the multiply and the store), near = looked-up rows whose norm is within
    1e-4 relative of max_norm (where float32 and float64 may disagree about the branch; the tests need 0)."""
    parts, bounds, near = [], [], 0
    for i, tb in enumerate(tables):
        rows = tb.double()[x[:, i]]
        norm = rows.norm(dim=1, keepdim=True)
        if max_norm > 0:
            near += int(((norm - max_norm).abs() <= 1e-4 * max_norm).sum())
            rows = t.where(norm > max_norm, rows * (max_norm / (norm + 1e-7)), rows)
        parts.append(rows)
        bounds.append((tb.shape[1] / 2 + 4) * U * rows.abs())
    return t.cat(parts, 1), t.cat(bounds, 1), near


def embed_emulate(x, tables, max_norm, bad_norm=False):
    """NumPy float32: sequential float32 sum of squares, sqrt, one divide, one multiply per element.  bad_norm=True takes the
    norm from the row truncated to bfloat16 (8 bits of precision): the deliberately worse emulation."""
    outs = []
    for i, tb in enumerate(tables):
        rows = tb.numpy()[x[:, i].numpy()]
        src = rows
        if bad_norm:
            src = (rows.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
        ss = np.zeros(rows.shape[0], F32)
        for k in range(rows.shape[1]):
            ss = ss + src[:, k] * src[:, k]
        norm = np.sqrt(ss)
        scale = np.where((max_norm > 0) & (norm > F32(max_norm)), F32(max_norm) / (norm + F32(1e-7)), F32(1))
        outs.append(rows * scale[:, None].astype(F32))
    return t.from_numpy(np.concatenate(outs, 1))


# ------------------------------------------------------------------------------------------------------------ segment max
SEG_WIDTHS = (1, 63, 64, 65, 129)
SEG_DSTS = (1, 5, 203)
SEG_SRC = 40


def segmax_case(n_dst, d, seed=0):
    """(src, dst, X, dY) for a bipartite relation of SEG_SRC sources.
    Sources: X[7] = X[9] = X[2] exactly (ties); rows 11, 12 are -inf; rows 13, 14 are < -1; the rest randn.
    Sources 7 and 9 appear only in segments that also hold 2, so they never win.
    n_dst = 1: the one segment holds {2, 7, 9, 13}.  n_dst = 5: 0 and 4 empty, 1 = {9, 7, 2} (+ duplicate edges), 2 = {12, 11}
    (all -inf), 3 = {14, 13} (all negative).  n_dst = 203: 0 and 202 empty; r % 4 == 1 as segment 1 plus a few random sources;
    r % 16 == 2: {11, 12}; r % 16 == 6: {13, 14}; r % 16 == 10: {11, 13} (a finite value beside -inf); others random;
    the first 60 edges are listed twice."""
    g = t.Generator().manual_seed(97 * n_dst + d + seed)
    X = t.randn(SEG_SRC, d, generator=g)
    X[2] += 2.5                                        # the tied value is the maximum of most segments that hold it
    X[7], X[9] = X[2], X[2]
    X[11:13] = float("-inf")
    X[13:15] = -1.0 - t.randn(2, d, generator=g).abs()
    plain = [s for s in range(SEG_SRC) if s not in (2, 7, 9, 11, 12, 13, 14)]
    edges = []
    if n_dst == 1:
        edges += [(0, s) for s in (13, 9, 2, 7)]
    for r in range(1, n_dst - 1):
        if n_dst == 5:
            srcs = {1: [9, 7, 2, 7], 2: [12, 11], 3: [14, 13]}[r]
        elif r % 4 == 1:
            srcs = [9, 7, 2] + [plain[int(i)] for i in t.randint(0, len(plain), (3,), generator=g)]
        elif r % 16 in (2, 6, 10):
            srcs = {2: [11, 12], 6: [13, 14], 10: [13, 11]}[r % 16]
        else:
            srcs = [plain[int(i)] for i in t.randint(0, len(plain), (int(t.randint(1, 9, (1,), generator=g)),), generator=g)]
        edges += [(r, s) for s in srcs]
    edges += edges[:60]
    order = t.randperm(len(edges), generator=g)
    e = t.tensor(edges, dtype=t.int64)[order]
    return e[:, 1].contiguous(), e[:, 0].contiguous(), X, t.randn(n_dst, d, generator=g)


def segmax_ref(src, dst, X, n_dst):
    """Dense float64 restatement: Y[r] = max over the distinct sources of r (0 where there are none), arg = the SMALLEST source id
    attaining it (first maximum in sorted source order), -1 for none."""
    member = t.zeros(n_dst, X.shape[0], dtype=t.bool)
    member[dst, src] = True
    vals = t.where(member[:, :, None], X.double()[None], t.tensor(float("-inf"), dtype=t.float64))
    best = vals.amax(dim=1)
    hit = member[:, :, None] & (vals == best[:, None, :])
    arg = hit.int().argmax(dim=1)                      # argmax of 0/1 = first 1
    empty = ~member.any(dim=1)
    best[empty], arg[empty] = 0.0, -1
    return best, arg


def segmax_bwd_ref(arg, dY, n_src):
    """dX[s, c] = sum of dY[r, c] over the destinations whose arg-max at column c is s, in float64; bound = terms U sum|terms|
    (a sequential float32 sum of `terms` addends)."""
    n_dst, d = dY.shape
    valid = arg >= 0
    cols = t.arange(d)[None, :].expand(n_dst, d)
    idx = (arg[valid].long(), cols[valid])
    ref = t.zeros(n_src, d, dtype=t.float64).index_put_(idx, dY.double()[valid], accumulate=True)
    mass = t.zeros(n_src, d, dtype=t.float64).index_put_(idx, dY.double().abs()[valid], accumulate=True)
    terms = t.zeros(n_src, d, dtype=t.float64).index_put_(idx, t.ones(int(valid.sum()), dtype=t.float64), accumulate=True)
    return ref, terms * U * mass


# ------------------------------------------------------------------------------------------------------------ CSR builders
CSR_SHAPES = ((1, 2), (2, 1), (64, 64), (65, 64), (64, 65), (1024, 1025), (3, 65536), (3, 65537))
CSR_NNZ = 2000


def coo_case(n_rows, n_cols, variant, seed=0):
    """(row, col) int64.  Fewer than CSR_NNZ possible pairs: all of them.  variant "largest": entries at (n_rows - 1, n_cols - 1),
    (0, n_cols - 1) and (n_rows - 1, 0) planted, each twice.  variant "empty_ends" (n_rows >= 3): no entry in the first and last
    row.  Both: the first 40 entries are repeated at the end (duplicates far apart in input order), shuffled input order."""
    g = t.Generator().manual_seed(n_rows * 131 + n_cols + seed)
    if n_rows * n_cols <= CSR_NNZ:
        row, col = [v.reshape(-1) for v in t.meshgrid(t.arange(n_rows), t.arange(n_cols), indexing="ij")]
        keep = t.randperm(row.numel(), generator=g)
        row, col = row[keep], col[keep]
    else:
        row, col = t.randint(0, n_rows, (CSR_NNZ,), generator=g), t.randint(0, n_cols, (CSR_NNZ,), generator=g)
    if variant == "largest":
        plant_r = t.tensor([n_rows - 1, 0, n_rows - 1] * 2)
        plant_c = t.tensor([n_cols - 1, n_cols - 1, 0] * 2)
        row, col = t.cat([plant_r[:3], row, plant_r[3:]]), t.cat([plant_c[:3], col, plant_c[3:]])
    else:
        assert variant == "empty_ends" and n_rows >= 3
        row = row.clamp(1, n_rows - 2)
    return t.cat([row, row[:40]]).contiguous(), t.cat([col, col[:40]]).contiguous()
