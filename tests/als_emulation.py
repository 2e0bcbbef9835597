"""The iALS rule of include/laplace_hip.h in numpy: its float64 evaluation, the (halved) objective, the accuracy bound a
float32 solution must meet, and an f32 Cholesky that serves as a reference implementation the bound is checked against.

Notation of the bound:  u = 2^-24,  g(k) = k u / (1 - k u)  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).
A row has entries e_0 .. e_{n-1} (y_e = Y[idx[e], :], float32), A = G + alpha * sum_e y_e y_e^T + reg I, b = (1 + alpha) sum_e y_e;
alpha and reg are the float32 values the kernel receives.

Forming.  The kernel's S[j][k] is a chain of fmaf over at most L entries per chunk and then one addition per further chunk:
    at most n roundings on any path, each of relative size u, so |S^ - S| <= g(n) sum_e |y_e[j]| |y_e[k]| (Higham Lemma 3.1, 3.3).
    A^ = fmaf(alpha, S^, G) (one rounding) and, on the diagonal, + reg (one more):
        |A^ - A| <= g(n + 2) (alpha * sum_e |y_e||y_e|^T + |G| + reg I)                                        =: E_A
    s^ needs n - 1 additions, (1.0f + alpha) one rounding, the product one:
        |b^ - b| <= g(n + 1) (1 + alpha) sum_e |y_e|                                                            =: E_b
Solving.  Cholesky followed by two triangular solves is backward stable whatever the order of its additions (Higham Theorems
    10.3 and 10.4): the computed factor R satisfies R^T R = A^ + dA1 with |dA1| <= g(d + 1) |R^T||R|, and the computed x
    satisfies (A^ + dA) x = b^ with |dA| <= g(3 d + 1) |R^T||R|.  The kernel scales a column by a ROUNDED RECIPROCAL of the
    square root (l = a * fl(1 / fl(sqrt(p)))) where the textbook divides (l = a / fl(sqrt(p))): one rounding more per element
    of R and of y; three more are allowed for here, g(d + 2) and g(3 d + 4).
    Norm of |R^T||R|:  || |R^T||R| ||_2 <= || |R| ||_F^2 = trace(R^T R) = trace(A^) + trace(dA1) <= trace(A^) + g(d + 2) ||R||_F^2,
    hence ||R||_F^2 <= trace(A^) / (1 - g(d + 2)) and
        ||dA||_2 <= g(3 d + 4) trace(A^) / (1 - g(d + 2))                                                        =: T
    Higham's eq. 10.7 continues with trace(A) <= d ||A||_2, which gives the familiar c_d ||A||_2 with
    c_d = d g(3 d + 1) / (1 - d g(d + 1)); the trace is kept here because it is the sharper of the two, by the factor
    d ||A||_2 / trace(A) — at d = 128 c_d alone is 2.9e-3, and a bound that loose could not tell a solution from one that is
    off by a relative 1e-3 (test_als_cpu.py asserts that this one can, on systems whose b lies near the dominant eigenvector).
Together, for the float64 A and b of the same row:
        b - A x = (b - b^) + (A^ - A) x + dA x
        ||b - A x||_2 <= ||E_b||_2 + (||E_A||_F + T) ||x||_2,        trace(A^) <= trace(A) + trace(E_A).
Nothing in this is fitted to a kernel's output.

Objective slack.  With the other table fixed, a row's share of the halved objective is f(x) = 1/2 x^T A x - b^T x + const, whose
minimiser is x* = A^-1 b.  For any x with residual r = b - A x:  f(x) - f(x*) = 1/2 r^T A^-1 r <= ||r||^2 / (2 reg), since
A - reg I is positive semi-definite.  A half-sweep that leaves residuals r_row can therefore end at most
sum_rows ||r_row||^2 / (2 reg) above the half-sweep's exact minimum, which is itself at most the previous objective.
"""
import numpy as np

U = 2.0 ** -24


def g(k):
    return k * U / (1.0 - k * U)


def solve_term(d, trace_a):
    """T of the docstring: the 2-norm of the solve's backward error."""
    return g(3 * d + 4) * trace_a / (1.0 - g(d + 2))


def system64(entries, Y, G, alpha, reg):
    """(A64, b64) of one row: entries are column ids in CSR order, a repeated id counts every time it occurs."""
    alpha, reg = float(np.float32(alpha)), float(np.float32(reg))
    R = np.asarray(Y, dtype=np.float64)[np.asarray(entries, dtype=np.int64)]
    d = Y.shape[1]
    A = np.asarray(G, dtype=np.float64) + alpha * (R.T @ R) + reg * np.eye(d)
    b = (1.0 + alpha) * R.sum(axis=0)
    return A, b


def x64(entries, Y, G, alpha, reg):
    if len(entries) == 0:
        return np.zeros(Y.shape[1])
    A, b = system64(entries, Y, G, alpha, reg)
    return np.linalg.solve(A, b)


def residual_bound(entries, Y, G, alpha, reg, x):
    """The right-hand side of the asserted inequality for a computed x of this row (see the module docstring)."""
    alpha, reg = float(np.float32(alpha)), float(np.float32(reg))
    n, d = len(entries), Y.shape[1]
    R = np.abs(np.asarray(Y, dtype=np.float64)[np.asarray(entries, dtype=np.int64)])
    E_A = g(n + 2) * (alpha * (R.T @ R) + np.abs(np.asarray(G, dtype=np.float64)) + reg * np.eye(d))
    E_b = g(n + 1) * (1.0 + alpha) * R.sum(axis=0)
    A, _ = system64(entries, Y, G, alpha, reg)
    ea = np.linalg.norm(E_A, "fro")
    T = solve_term(d, np.trace(A) + np.trace(E_A))
    return np.linalg.norm(E_b) + (ea + T) * np.linalg.norm(np.asarray(x, dtype=np.float64))


def residual(entries, Y, G, alpha, reg, x):
    A, b = system64(entries, Y, G, alpha, reg)
    return np.linalg.norm(b - A @ np.asarray(x, dtype=np.float64))


def form_f32(entries, Y, G, alpha, reg):
    """(A, b) in float32, entry by entry.  numpy has no fma: product and addition round separately, which the inner-product
    bound g(n) covers as well (Higham eq. 3.5), so E_A and E_b hold for this reference too."""
    alpha, reg = np.float32(alpha), np.float32(reg)
    d = Y.shape[1]
    S = np.zeros((d, d), dtype=np.float32)
    s = np.zeros(d, dtype=np.float32)
    for e in entries:
        y = Y[e].astype(np.float32)
        S = S + np.outer(y, y)
        s = s + y
    A = (alpha * S + G.astype(np.float32)).astype(np.float32)
    A[np.diag_indices(d)] += reg
    return A, ((np.float32(1.0) + alpha) * s).astype(np.float32)


def cholesky_solve_f32(A, b):
    """x of A x = b by a float32 Cholesky (column by column, every operation rounded to float32), forward and backward
    substitution.  Returns None at a pivot that is not a positive finite number."""
    A = np.array(A, dtype=np.float32)
    d = A.shape[0]
    Lm = np.zeros((d, d), dtype=np.float32)
    for k in range(d):
        p = A[k, k] - np.dot(Lm[k, :k], Lm[k, :k]).astype(np.float32) if k else A[k, k]
        p = np.float32(p)
        if not (p > 0 and np.isfinite(p)):
            return None
        Lm[k, k] = np.sqrt(p)
        if k + 1 < d:
            col = A[k + 1:, k] - (Lm[k + 1:, :k] @ Lm[k, :k]).astype(np.float32) if k else A[k + 1:, k]
            Lm[k + 1:, k] = (col.astype(np.float32) / Lm[k, k]).astype(np.float32)
    y = np.zeros(d, dtype=np.float32)
    for k in range(d):
        y[k] = (np.float32(b[k]) - np.dot(Lm[k, :k], y[:k]).astype(np.float32)) / Lm[k, k]
    x = np.zeros(d, dtype=np.float32)
    for k in range(d - 1, -1, -1):
        x[k] = (y[k] - np.dot(Lm[k + 1:, k], x[k + 1:]).astype(np.float32)) / Lm[k, k]
    return x


def objective(ptr, idx, X, Y, alpha, reg):
    """The halved iALS objective in float64 (als.ImplicitALS.objective): 1/2 sum over all pairs of c (p - x . y)^2 plus
    reg / 2 (|X|^2 + |Y|^2), c = 1 + alpha and p = 1 on every entry of the CSR, c = 1 and p = 0 elsewhere."""
    alpha, reg = float(np.float32(alpha)), float(np.float32(reg))
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    total = ((X @ (Y.T @ Y)) * X).sum()
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    s = (X[rows] * Y[np.asarray(idx, dtype=np.int64)]).sum(axis=1)
    total += ((1.0 + alpha) * (1.0 - s) ** 2 - s * s).sum()
    total += reg * ((X * X).sum() + (Y * Y).sum())
    return 0.5 * total


def objective_gradient_row(entries, Y, G, alpha, reg, x):
    """Gradient of the halved objective with respect to one row, the other table fixed: A x - b."""
    A, b = system64(entries, Y, G, alpha, reg)
    return A @ np.asarray(x, dtype=np.float64) - b


def half_sweep64(ptr, idx, Y, alpha, reg):
    """One float64 half-sweep: every row of the CSR solved against Y with G = Y^T Y."""
    Y = np.asarray(Y, dtype=np.float64)
    G = Y.T @ Y
    alpha, reg = float(alpha), float(reg)
    d = Y.shape[1]
    out = np.zeros((len(ptr) - 1, d))
    eye = reg * np.eye(d)
    for r in range(len(ptr) - 1):
        e = idx[ptr[r]:ptr[r + 1]]
        if len(e):
            R = Y[e]
            out[r] = np.linalg.solve(G + alpha * (R.T @ R) + eye, (1.0 + alpha) * R.sum(axis=0))
    return out


def csr_of(rows, cols, n_rows):
    """(ptr, idx) with the entries of a row in input order (a stable sort by row)."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=ptr[1:])
    return ptr, cols[order]


def map_at_k_single(scores, held_users, held_items, ptr, idx, k=12):
    """MAP@k with one held-out item per user: 1 / rank if the item is among the user's k best unseen items, else 0; ties go
    to the lower item id.  scores [n_held_users, n_items] float64, rows aligned with held_users."""
    ap = np.zeros(len(held_users))
    for p, (u, i) in enumerate(zip(held_users, held_items)):
        sc = scores[p].copy()
        sc[idx[ptr[u]:ptr[u + 1]]] = -np.inf
        rank = int((sc > sc[i]).sum() + (sc[:i] == sc[i]).sum())
        if rank < k:
            ap[p] = 1.0 / (rank + 1)
    return float(ap.mean())
