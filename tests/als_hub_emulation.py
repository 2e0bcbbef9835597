"""The "iALS block hub" rule of include/laplace_hip.h in numpy: a hub row's system is formed once (chunks of L_h entries, one
chain per chunk, chunks added in ascending order — the Cholesky solver's formation) and the block steps run on (A, b):
    u = A[pi, :] x,   g = u - b[pi],   H = A[pi, pi],   H delta = -g,   x[pi] += delta.
hub_sweep64 is its float64 evaluation, hub_sweep_f32 the same steps with every operation rounded to float32, and
hub_jacobi64 a deliberately WRONG schedule the tests' tolerance must tell from the rule.  conf=None is the unweighted rule
(alpha, reg); with conf (a_e per entry) alpha is not used and reg is the row's reg_r.

In exact arithmetic this is the block rule's own iteration: with p_e = y_e . x,
    sum_e w_e y_e[j] + (G x)[j] + reg x[j] = sum_e (alpha p_e - (1 + alpha)) y_e[j] + (G x)[j] + reg x[j] = (A x - b)[j],
and H is the same matrix.  tests/test_als_hub_cpu.py checks that against als_block_emulation / als_weighted_emulation.

Roundings of the formation, for the derived bounds (d <= B, zero start, one sweep: the one block step solves A x = b).  A and b
ARE the Cholesky entries' (als_emulation: E_A with g(n + 2), E_b with g(n + 1); als_weighted_emulation: g(n + 3), g(n + 1)).
With x = 0 the chains of u are sums of exact zeros, g = 0 - b = -b exactly and x = 0 + delta exactly, so
als_emulation.residual_bound / als_weighted_emulation.residual_bound hold as they stand.
"""
import numpy as np

import als_block_emulation as BE
import als_emulation as AE

F = np.float32


def _rows(entries, conf, Y, dtype):
    R = np.asarray(Y, dtype=dtype)[np.asarray(entries, dtype=np.int64)]
    a = None if conf is None else np.asarray(conf, dtype=F).astype(dtype)
    assert a is None or a.shape == (len(entries),)
    return R, a


def system64(entries, Y, G, alpha, reg, conf=None):
    """(A, b) of a row in float64, G read through its lower triangle."""
    alpha, reg = float(F(alpha)), float(F(reg))
    d = Y.shape[1]
    R, a = _rows(entries, conf, Y, np.float64)
    Gs = BE.sym_lower(np.asarray(G, dtype=np.float64))
    if a is None:
        return Gs + alpha * (R.T @ R) + reg * np.eye(d), (1.0 + alpha) * R.sum(axis=0)
    return Gs + (R * a[:, None]).T @ R + reg * np.eye(d), ((1.0 + a)[:, None] * R).sum(axis=0)


def hub_sweep64(entries, Y, G, alpha, reg, x0, B, sweeps, conf=None):
    """The hub rule in float64 from the start x0 (None: zero)."""
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d)
    A, b = system64(entries, Y, G, alpha, reg, conf)
    x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
    for _ in range(sweeps):
        for pi in BE.blocks(d, B):
            g = A[pi, :] @ x - b[pi]
            x[pi] += np.linalg.solve(A[pi, pi], -g)
    return x


def hub_jacobi64(entries, Y, G, alpha, reg, x0, B, sweeps, conf=None):
    """WRONG on purpose: every block of a sweep sees the x of the sweep's start."""
    d = Y.shape[1]
    if len(entries) == 0:
        return np.zeros(d)
    A, b = system64(entries, Y, G, alpha, reg, conf)
    x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
    for _ in range(sweeps):
        new = x.copy()
        for pi in BE.blocks(d, B):
            new[pi] = x[pi] + np.linalg.solve(A[pi, pi], -(A[pi, :] @ x - b[pi]))
        x = new
    return x


def form_f32(entries, Y, G, alpha, reg, L, conf=None, panel=64):
    """(A, b) in float32 by the rule: per chunk of L entries one chain per element (numpy has no fma: product and addition
    round separately), chunks added in ascending order, then the system line; A(j, k) = A[max][min].  The chains of a chunk
    are made `panel` columns at a time (32 MiB at d = 256 and 512 entries): a 2 049-entry chunk at d = 256 made whole would be
    half a gigabyte."""
    alpha, reg = F(alpha), F(reg)
    d = Y.shape[1]
    R, a = _rows(entries, conf, Y, F)
    Z = R if a is None else (R * a[:, None]).astype(F)
    Cw = R if a is None else ((F(1.0) + a).astype(F)[:, None] * R).astype(F)
    S = s = None
    for c0 in range(0, len(entries), L):
        Rc, Zc = R[c0:c0 + L], Z[c0:c0 + L]
        Sc = np.zeros((d, d), dtype=F)
        for k0 in range(0, d, panel):
            Sc[:, k0:k0 + panel] = BE._chain(Rc[:, :, None] * Zc[:, None, k0:k0 + panel], 0)
        sc = BE._chain(Cw[c0:c0 + L], 0)
        S, s = (Sc, sc) if S is None else ((S + Sc).astype(F), (s + sc).astype(F))
    Gf = np.asarray(G, dtype=F)
    A = ((alpha * S).astype(F) + Gf).astype(F) if a is None else (Gf + S).astype(F)
    A = np.tril(A) + np.tril(A, -1).T
    A[np.diag_indices(d)] += reg
    b = ((F(1.0) + alpha) * s).astype(F) if a is None else s
    return A.astype(F), b.astype(F)


def _u_f32(Ap, x, B):
    """u[j] = sum_k A(j, k) x[k] in the chain layout of the block rule's q: 64 / B chains over groups of four columns."""
    d, jg = x.shape[0], 64 // B
    u = None
    for m in range(jg):
        cols = np.concatenate([np.arange(4 * g, 4 * g + 4) for g in range(m, d // 4, jg)] or [np.zeros(0, dtype=np.int64)])
        ch = BE._chain(Ap[:, cols] * x[None, cols], 1) if len(cols) else np.zeros(Ap.shape[0], dtype=F)
        u = ch if u is None else (u + ch).astype(F)
    return u


def steps_f32(A, b, x0, B, sweeps):
    """The block steps on an assembled float32 system.  None at a failed pivot."""
    d = A.shape[0]
    x = np.zeros(d, dtype=F) if x0 is None else np.array(x0, dtype=F)
    for _ in range(sweeps):
        for pi in BE.blocks(d, B):
            g = (_u_f32(A[pi, :], x, B) - b[pi]).astype(F)
            delta = AE.cholesky_solve_f32(A[pi, pi], -g)
            if delta is None:
                return None
            x[pi] = x[pi] + delta
    return x


def hub_sweep_f32(entries, Y, G, alpha, reg, x0, B, sweeps, L, conf=None):
    """The hub rule with every operation rounded to float32.  None at a failed pivot."""
    if len(entries) == 0:
        return np.zeros(Y.shape[1], dtype=F)
    A, b = form_f32(entries, Y, G, alpha, reg, L, conf)
    return steps_f32(A, b, x0, B, sweeps)
