"""The weighted iALS rules of include/laplace_hip.h ("iALS weighted", "iALS block weighted") in numpy: their float64
evaluation, float32 references, the (halved) weighted objective, the per-row regulariser of als.ImplicitALS, and the accuracy
bound a float32 solution must meet.  The unweighted modules als_emulation (AE) and als_block_emulation (BE) supply g(k), the
solve term, the float32 Cholesky and the block helpers.

A row has entries e_0 .. e_{n-1} (y_e = Y[idx[e], :], float32) with a_e = conf[e] >= 0 (float32) and a regulariser reg_r
(float32):
    A = G + sum_e a_e y_e y_e^T + reg_r I,        b = sum_e (1 + a_e) y_e.

The bound: als_emulation's derivation redone for the weighted formation (u = 2^-24, g(k) = k u / (1 - k u)).
Forming A.  z_e[k] = fl(a_e y_e[k]) is one rounding: z^ = a_e y_e[k] (1 + t), |t| <= u.  S^[j][k] is a chain of fmaf(y_e[j],
    z^_e[k], acc) over at most L entries per chunk and then one addition per further chunk: as in the unweighted rule at most n
    roundings on any path from a product to the sum, and the product now carries the one of z^: n + 1 factors (1 + t_i), so
        |S^ - S| <= g(n + 1) sum_e a_e |y_e[j]| |y_e[k]|                                        (Higham Lemma 3.1, 3.3).
    A^ = fl(G + S^) is ONE further rounding of the whole sum (the unweighted rule has fmaf(alpha, S^, G) there, also one), and
    on the diagonal + reg_r is one more.  Every term of A therefore carries at most n + 3 roundings, G's at most 2 and reg_r's 1:
        |A^ - A| <= g(n + 3) (sum_e a_e |y_e||y_e|^T + |G| + reg_r I)                                              =: E_A
Forming b.  c^_e = fl(1 + a_e) is one rounding.  s^[j] is a chain of n fmaf(c^_e, y_e[j], acc) from 0, one rounding each (the
    first is not exact here: it rounds the product), chunks added in order: again at most n roundings on any path, so with c^'s
        |b^ - b| <= g(n + 1) sum_e (1 + a_e) |y_e|                                                                  =: E_b
    (the unweighted rule reaches the same count by n - 1 additions, the rounding of 1 + alpha and the product).
    The float32 REFERENCE below has no fma: y z rounds separately from the addition.  The first addition (to 0) is then exact
    and every later path is one shorter, so a term still meets n + 1 roundings in S^ (z, the product, at most n - 1 additions)
    and n + 1 in s^ (c, the product, n - 1 additions): E_A and E_b hold for it unchanged (Higham eq. 3.5).
Solving.  Unchanged: (A^ + dA) x = b^ with ||dA||_2 <= T = g(3 d + 4) trace(A^) / (1 - g(d + 2)), trace(A^) <= trace(A) + trace(E_A).
Together     ||b - A x||_2 <= ||E_b||_2 + (||E_A||_F + T) ||x||_2.
Block form with d <= B, a zero start and one sweep: H = fl(G + S^) + reg_r makes the same n + 3 roundings; p = 0 gives
    w_e = fmaf(a_e, 0, -c^_e) = -c^_e exactly, q = 0 and fmaf(reg_r, 0, gs + 0) = gs exactly, and gs is a chain of n fmaf over
    c^_e: the n + 1 roundings of E_b.  x = 0 + delta is exact.  The bound holds as it stands.
Nothing in this is fitted to a kernel's output.

Objective slack.  As in als_emulation: f(x) - f(x*) = 1/2 r^T A^-1 r <= ||r||^2 / (2 reg_r) <= ||r||^2 / (2 min_r reg_r).
"""
import numpy as np

import als_block_emulation as BE
import als_emulation as AE

F = np.float32


def _rows(entries, conf, Y, dtype=np.float64):
    R = np.asarray(Y, dtype=dtype)[np.asarray(entries, dtype=np.int64)]
    a = np.asarray(conf, dtype=F).astype(dtype)
    assert a.shape == (len(entries),)
    return R, a


# ---- the Cholesky form ----------------------------------------------------------------------------------------------------------
def system64(entries, conf, Y, G, reg_r):
    """(A64, b64) of one row: entries are column ids in CSR order, conf their a_e; a repeated id counts every time."""
    R, a = _rows(entries, conf, Y)
    d = Y.shape[1]
    A = np.asarray(G, dtype=np.float64) + (R * a[:, None]).T @ R + float(F(reg_r)) * np.eye(d)
    b = ((1.0 + a)[:, None] * R).sum(axis=0)
    return A, b


def x64(entries, conf, Y, G, reg_r):
    if len(entries) == 0:
        return np.zeros(Y.shape[1])
    A, b = system64(entries, conf, Y, G, reg_r)
    return np.linalg.solve(A, b)


def residual(entries, conf, Y, G, reg_r, x):
    A, b = system64(entries, conf, Y, G, reg_r)
    return np.linalg.norm(b - A @ np.asarray(x, dtype=np.float64))


def residual_bound(entries, conf, Y, G, reg_r, x):
    """The right-hand side of the asserted inequality for a computed x of this row (see the module docstring)."""
    n, d = len(entries), Y.shape[1]
    R, a = _rows(entries, conf, Y)
    R = np.abs(R)
    E_A = AE.g(n + 3) * ((R * a[:, None]).T @ R + np.abs(np.asarray(G, dtype=np.float64)) + float(F(reg_r)) * np.eye(d))
    E_b = AE.g(n + 1) * ((1.0 + a)[:, None] * R).sum(axis=0)
    A, _ = system64(entries, conf, Y, G, reg_r)
    T = AE.solve_term(d, np.trace(A) + np.trace(E_A))
    return np.linalg.norm(E_b) + (np.linalg.norm(E_A, "fro") + T) * np.linalg.norm(np.asarray(x, dtype=np.float64))


def form_f32(entries, conf, Y, G, reg_r):
    """(A, b) in float32 by the rule's steps, entry by entry (numpy has no fma: product and addition round separately)."""
    d = Y.shape[1]
    S = np.zeros((d, d), dtype=F)
    s = np.zeros(d, dtype=F)
    for e, a in zip(entries, np.asarray(conf, dtype=F)):
        y = Y[e].astype(F)
        z = (a * y).astype(F)
        S = S + np.outer(y, z).astype(F)
        s = s + ((F(1.0) + a) * y).astype(F)
    A = (G.astype(F) + S).astype(F)
    A[np.diag_indices(d)] += F(reg_r)
    return A, s


def x_f32(entries, conf, Y, G, reg_r):
    """The float32 reference solution (None at a failed pivot)."""
    if len(entries) == 0:
        return np.zeros(Y.shape[1], dtype=F)
    A, b = form_f32(entries, conf, Y, G, reg_r)
    return AE.cholesky_solve_f32(A, b)


def objective_gradient_row(entries, conf, Y, G, reg_r, x):
    """Gradient of the halved weighted objective with respect to one row, the other table fixed: A x - b."""
    A, b = system64(entries, conf, Y, G, reg_r)
    return A @ np.asarray(x, dtype=np.float64) - b


# ---- the block form -------------------------------------------------------------------------------------------------------------
def block_sweep64(entries, conf, Y, G, reg_r, x0, B, sweeps):
    """The block rule in float64 from the start x0 (None: zero)."""
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d)
    reg_r = float(F(reg_r))
    R, a = _rows(entries, conf, Y)
    Gs = BE.sym_lower(np.asarray(G, dtype=np.float64))
    x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
    p = R @ x
    for _ in range(sweeps):
        for pi in BE.blocks(d, B):
            w = a * p - (1.0 + a)
            g = R[:, pi].T @ w + Gs[pi, :] @ x + reg_r * x[pi]
            H = Gs[pi, pi] + (R[:, pi] * a[:, None]).T @ R[:, pi] + reg_r * np.eye(pi.stop - pi.start)
            delta = np.linalg.solve(H, -g)
            x[pi] += delta
            p += R[:, pi] @ delta
    return x


def block_sweep_f32(entries, conf, Y, G, reg_r, x0, B, sweeps):
    """The block rule with every operation rounded to float32 (no fma; every sum one chain in ascending order;
    als_emulation.cholesky_solve_f32 for the small systems).  None at a failed pivot."""
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d, dtype=F)
    reg_r = F(reg_r)
    R, a = _rows(entries, conf, Y, F)
    Gs = BE.sym_lower(np.asarray(G, dtype=F))
    x = np.zeros(d, dtype=F) if x0 is None else np.array(x0, dtype=F)
    c = (F(1.0) + a).astype(F)
    p = np.zeros(len(entries), dtype=F) if x0 is None else BE._chain(R * x[None, :], 1)
    for _ in range(sweeps):
        for pi in BE.blocks(d, B):
            Rp = R[:, pi]
            Zp = (Rp * a[:, None]).astype(F)
            w = ((a * p).astype(F) - c).astype(F)
            q = BE._chain(Gs[pi, :] * x[None, :], 1)
            gs = BE._chain(Rp * w[:, None], 0)
            g = ((gs + q).astype(F) + (reg_r * x[pi]).astype(F)).astype(F)
            S = BE._chain(Rp[:, :, None] * Zp[:, None, :], 0)
            H = (Gs[pi, pi] + S).astype(F)
            H[np.diag_indices(H.shape[0])] += reg_r
            delta = AE.cholesky_solve_f32(H, -g)
            if delta is None:
                return None
            x[pi] = x[pi] + delta
            p = p + BE._chain(Rp * delta[None, :], 1)
    return x


# ---- the model's side -----------------------------------------------------------------------------------------------------------
def reg_rows64(ptr, conf, n_cols, reg, nu):
    """reg_r = reg * (n_cols + sum_e a_e)^nu per row of a CSR, in float64 (als.reg_rows_of rounds it to float32)."""
    a = np.asarray(conf, dtype=F).astype(np.float64)
    mass = np.array([a[ptr[r]:ptr[r + 1]].sum() for r in range(len(ptr) - 1)])
    return float(reg) * (float(n_cols) + mass) ** float(nu)


def objective(ptr, idx, conf, X, Y, reg_u, reg_i):
    """The halved weighted objective in float64 (als.ImplicitALS.objective): 1/2 sum over all pairs of c (p - x . y)^2 plus
    1/2 (sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2), c = 1 + a_e and p = 1 on every entry of the CSR, c = 1 and p = 0
    elsewhere.  reg_u / reg_i: a scalar or one value per row."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    a = np.asarray(conf, dtype=F).astype(np.float64)
    total = ((X @ (Y.T @ Y)) * X).sum()
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    s = (X[rows] * Y[np.asarray(idx, dtype=np.int64)]).sum(axis=1)
    total += ((1.0 + a) * (1.0 - s) ** 2 - s * s).sum()
    total += (np.asarray(reg_u, dtype=np.float64) * (X * X).sum(axis=1)).sum()
    total += (np.asarray(reg_i, dtype=np.float64) * (Y * Y).sum(axis=1)).sum()
    return 0.5 * total
