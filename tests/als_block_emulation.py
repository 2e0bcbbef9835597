"""The iALS block rule of include/laplace_hip.h in numpy: its float64 evaluation (block_sweep64), the same steps with every
operation rounded to float32 (block_sweep_f32: the yardstick the kernel's distance from float64 is measured against), and a
deliberately WRONG variant (jacobi_sweep64) that the tests' tolerance must be able to tell from the rule.

A row has entries e_0 .. e_{n-1} (y_e = Y[idx[e], :]), A = G + alpha * sum_e y_e y_e^T + reg I and b = (1 + alpha) sum_e y_e as in
tests/als_emulation.py; its share of the halved objective is f(x) = 1/2 x^T A x - b^T x.  With p_e = y_e . x,
    grad f (x)[j] = sum_e (alpha p_e - (1 + alpha)) y_e[j] + (G x)[j] + reg x[j],        hess f [j][k] = A[j][k],
so a block step  x[pi] += H^-1 (-g)  with H = A[pi, pi] and g = grad f(x)[pi] is the exact minimiser of f over x[pi].

Roundings of the formation, for the derived bound of als_emulation.residual_bound (d <= B, zero start, one sweep: the one
block step solves A x = b).  H = fmaf(alpha, S, G) + reg with S a chain of n fmaf: n + 2 roundings, E_A's g(n + 2).  With x = 0
and p = 0: w_e = -(1.0f + alpha) (one rounding), q = 0 and reg x = 0 exactly, so -g[j] = -sum_e fmaf(y_e[j], w, acc) is n + 1
roundings: E_b's g(n + 1).  x = 0 + delta is exact.  The bound therefore holds as it stands.
"""
import numpy as np

import als_emulation as AE

F = np.float32


def sym_lower(G):
    """G(j, k) = G[max(j, k)][min(j, k)]: the matrix the rule reads."""
    G = np.asarray(G)
    return np.tril(G) + np.tril(G, -1).T


def blocks(d, B):
    return [slice(c0, min(c0 + B, d)) for c0 in range(0, d, B)]


def block_sweep64(entries, Y, G, alpha, reg, x0, B, sweeps, hook=None):
    """The rule in float64 from the start x0 (None: zero).  hook(x) is called after every block step."""
    alpha, reg = float(F(alpha)), float(F(reg))
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d)
    R = np.asarray(Y, dtype=np.float64)[np.asarray(entries, dtype=np.int64)]
    Gs = sym_lower(np.asarray(G, dtype=np.float64))
    x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
    p = R @ x
    for _ in range(sweeps):
        for pi in blocks(d, B):
            w = alpha * p - (1.0 + alpha)
            g = R[:, pi].T @ w + Gs[pi, :] @ x + reg * x[pi]
            H = Gs[pi, pi] + alpha * (R[:, pi].T @ R[:, pi]) + reg * np.eye(pi.stop - pi.start)
            delta = np.linalg.solve(H, -g)
            x[pi] += delta
            p += R[:, pi] @ delta
            if hook is not None:
                hook(x.copy())
    return x


def jacobi_sweep64(entries, Y, G, alpha, reg, x0, B, sweeps):
    """WRONG on purpose: every block of a sweep sees the x and p of the sweep's start."""
    alpha, reg = float(F(alpha)), float(F(reg))
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d)
    R = np.asarray(Y, dtype=np.float64)[np.asarray(entries, dtype=np.int64)]
    Gs = sym_lower(np.asarray(G, dtype=np.float64))
    x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
    for _ in range(sweeps):
        p = R @ x
        w = alpha * p - (1.0 + alpha)
        new = x.copy()
        for pi in blocks(d, B):
            g = R[:, pi].T @ w + Gs[pi, :] @ x + reg * x[pi]
            H = Gs[pi, pi] + alpha * (R[:, pi].T @ R[:, pi]) + reg * np.eye(pi.stop - pi.start)
            new[pi] = x[pi] + np.linalg.solve(H, -g)
        x = new
    return x


def _chain(prod, axis):
    """A float32 chain acc = acc + prod[i] in ascending i (np.add.accumulate is strictly sequential)."""
    return np.add.accumulate(prod.astype(F), axis=axis, dtype=F).take(-1, axis=axis)


def block_sweep_f32(entries, Y, G, alpha, reg, x0, B, sweeps):
    """The rule with every operation rounded to float32 (numpy has no fma: product and addition round separately; every sum a
    single chain in ascending order; als_emulation.cholesky_solve_f32 for the small systems).  None at a failed pivot."""
    alpha, reg = F(alpha), F(reg)
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d, dtype=F)
    R = np.asarray(Y, dtype=F)[np.asarray(entries, dtype=np.int64)]
    Gs = sym_lower(np.asarray(G, dtype=F))
    x = np.zeros(d, dtype=F) if x0 is None else np.array(x0, dtype=F)
    c1 = -(F(1.0) + alpha)
    p = np.zeros(len(entries), dtype=F) if x0 is None else _chain(R * x[None, :], 1)
    for _ in range(sweeps):
        for pi in blocks(d, B):
            Rp = R[:, pi]
            w = alpha * p + c1
            q = _chain(Gs[pi, :] * x[None, :], 1)
            gs = _chain(Rp * w[:, None], 0)
            g = (gs + q) + reg * x[pi]
            S = _chain(Rp[:, :, None] * Rp[:, None, :], 0)
            H = alpha * S + Gs[pi, pi]
            H[np.diag_indices(H.shape[0])] += reg
            delta = AE.cholesky_solve_f32(H, -g)
            if delta is None:
                return None
            x[pi] = x[pi] + delta
            p = p + _chain(Rp * delta[None, :], 1)
    return x


def row_share64(entries, Y, G, alpha, reg, x):
    """f(x) = 1/2 x^T A x - b^T x of one row, G read through its lower triangle."""
    A, b = AE.system64(entries, Y, sym_lower(np.asarray(G, dtype=np.float64)), alpha, reg)
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x @ A @ x - b @ x


def half_sweep(fn, ptr, idx, Y, G, alpha, reg, X0, B, sweeps):
    """fn (one of the sweeps above) on every row of a CSR from the rows of X0."""
    out = np.zeros((len(ptr) - 1, Y.shape[1]), dtype=np.float64)
    for r in range(len(ptr) - 1):
        out[r] = fn(idx[ptr[r]:ptr[r + 1]], Y, G, alpha, reg, None if X0 is None else X0[r], B, sweeps)
    return out
