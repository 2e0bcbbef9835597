"""Inputs shared by tests/test_als_weighted_cpu.py and tests/test_gpu_als_weighted.py (numpy only): the weighted problems of the
GPU test with their float64 and float32 references, computed once per process, and the two exact cases."""
import numpy as np

import als_block_cases as BC
import als_weighted_emulation as WE
from laplace_amd import ops

ALPHA, REG = BC.ALPHA, BC.REG            # the constant-weights comparison with the unweighted rule
N_COLS = BC.N_COLS
CHOL_DIMS = (16, 64, 128)
BLOCK_SHAPES = ((40, 16), (128, 32), (256, 64))          # several blocks: the float32 yardstick
ONE_BLOCK_SHAPES = ((16, 16), (64, 64))                  # d <= B: the derived bound
STARTS = ((True, 1), (False, 3))                         # (from zero, sweeps)
REPEAT_ROW, ZERO_ROW = 8, 9                              # a repeated entry; some a_e == 0


def _weights(rng, rows):
    """a_e log-uniform in [0.1, 30] per entry, reg_rows uniform in [0.5, 5] per row, both float32."""
    conf = [np.exp(rng.uniform(np.log(0.1), np.log(30.0), len(e))).astype(np.float32) for e in rows]
    reg_rows = rng.uniform(0.5, 5.0, len(rows)).astype(np.float32)
    return conf, reg_rows


def _special_rows(rng, rows, conf):
    rows[REPEAT_ROW] = [11, 42, 7, 42, 3, 250]
    conf[REPEAT_ROW] = conf[REPEAT_ROW][:1].repeat(6) * np.float32([1, 2, 0.5, 3, 1, 1])
    rows[ZERO_ROW] = rng.integers(0, N_COLS, 12).tolist()
    conf[ZERO_ROW] = np.exp(rng.uniform(np.log(0.1), np.log(30.0), 12)).astype(np.float32)
    conf[ZERO_ROW][::3] = 0.0


class CholProblem:
    """One width of the Cholesky form: rows of lengths 0, 1, 3, 33, L - 1, L + 1 and 2 L + 5 (L = ops.als_chunk(d)), a
    row with a repeated entry, one with some a_e == 0 and random short ones, over a column slice (ldy = d + 8) of a wider
    table whose rows share an offset."""
    LONG_ROW, N_ROWS = 6, 20

    def __init__(self, d):
        rng = np.random.default_rng(7000 + d)
        self.d, self.L = d, ops.als_chunk(d)
        L = self.L
        lens = [0, 1, 3, 33, L - 1, L + 1, 2 * L + 5, 5, 5, 5]
        lens += rng.integers(1, 40, self.N_ROWS - len(lens)).tolist()
        self.rows = [rng.integers(0, N_COLS, n).tolist() for n in lens]
        self.conf, self.reg_rows = _weights(rng, self.rows)
        _special_rows(rng, self.rows, self.conf)
        self.wide = (0.25 + rng.standard_normal((N_COLS, d + 8)) * 0.2).astype(np.float32)
        self.Y = self.wide[:, 4:4 + d]
        G = self.Y.astype(np.float64).T @ self.Y.astype(np.float64)
        self.G = np.tril(G.astype(np.float32))
        self.G = self.G + np.tril(self.G, -1).T
        self._x32 = None

    def x32(self):
        """The float32 reference solution of every row."""
        if self._x32 is None:
            self._x32 = [WE.x_f32(e, a, self.Y, self.G, self.reg_rows[r]) for r, (e, a) in enumerate(zip(self.rows, self.conf))]
        return self._x32

    def check_row(self, r, x, tag=""):
        """x of row r is inside the derived residual bound (an empty row: exactly zero)."""
        e, a, reg_r = self.rows[r], self.conf[r], self.reg_rows[r]
        if len(e) == 0:
            assert not np.asarray(x).any(), r
            return
        assert np.isfinite(x).all(), r
        res, bound = WE.residual(e, a, self.Y, self.G, reg_r, x), WE.residual_bound(e, a, self.Y, self.G, reg_r, x)
        print(f"{tag}d={self.d} row {r} n={len(e)}: residual {res:.3e} bound {bound:.3e}")
        assert res <= bound, (self.d, r, len(e), res, bound)


class BlockProblem:
    """One (d, B) of the block form: als_block_cases.Problem's table, G, start and rows (lengths 0, 1, 3, B - 1, B + 1, 33,
    70, chunk + 5 and random short ones; ldy = d + 8), two of the random rows replaced by the repeated-entry and the
    zero-weight row, with weights per entry and a regulariser per row."""
    LONG_ROW, N_ROWS = BC.LONG_ROW, BC.N_ROWS

    def __init__(self, d, B):
        base = BC.problem(d, B)
        rng = np.random.default_rng(9000 * d + B)
        self.d, self.B, self.chunk = d, B, base.chunk
        self.rows = [list(e) for e in base.rows]
        self.conf, self.reg_rows = _weights(rng, self.rows)
        _special_rows(rng, self.rows, self.conf)
        self.wide, self.Y, self.G, self.X0 = base.wide, base.Y, base.G, base.X0
        self._refs = {}

    def refs(self, from_zero, sweeps):
        """(X64, X32, tol): the rule in float64, the float32 reference, and 8 * max_r ||x_f32ref - x_64||_2."""
        key = (from_zero, sweeps)
        if key not in self._refs:
            X64 = np.zeros((self.N_ROWS, self.d))
            X32 = np.zeros((self.N_ROWS, self.d), dtype=np.float32)
            for r, (e, a) in enumerate(zip(self.rows, self.conf)):
                x0 = None if from_zero else self.X0[r]
                X64[r] = WE.block_sweep64(e, a, self.Y, self.G, self.reg_rows[r], x0, self.B, sweeps)
                X32[r] = WE.block_sweep_f32(e, a, self.Y, self.G, self.reg_rows[r], x0, self.B, sweeps)
            tol = 8.0 * np.linalg.norm(X32.astype(np.float64) - X64, axis=1).max()
            self._refs[key] = (X64, X32, tol)
        return self._refs[key]


_PROBLEMS = {}


def chol_problem(d):
    if d not in _PROBLEMS:
        _PROBLEMS[d] = CholProblem(d)
    return _PROBLEMS[d]


def block_problem(d, B):
    if (d, B) not in _PROBLEMS:
        _PROBLEMS[(d, B)] = BlockProblem(d, B)
    return _PROBLEMS[(d, B)]


def csr_arrays(rows, conf):
    """(ptr int32, idx int32, conf float32) of a list of rows."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    if ptr[-1] == 0:
        return ptr, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    return ptr, np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]), np.concatenate(conf).astype(np.float32)


# (a_e, |entry| factor) of the three item groups: a_e * factor^2 == 1, so the weighted diagonal is the unweighted one
_EXACT_GROUPS = ((1.0, 1.0), (4.0, 0.5), (0.25, 2.0))


def exact_chol_case():
    """d = 16.  One-hot item rows: the item (j, c) of column j and group c holds +-mag_j * f_c and carries a_e = a_c, with
    a_c f_c^2 = 1 (powers of two), so A = diag(G_jj + mag_j^2 + reg) whatever the groups a row draws from; G_jj is chosen so
    that every A_jj is a power of FOUR with reg = 1.  Every operation of the rule and of the factorisation is exact:
    x_j = (1 + a_e) y_e[j] / A_jj bit for bit.  Returns (Y, G, rows, conf, reg_rows)."""
    d = 16
    rng = np.random.default_rng(7)
    mag = np.array([1, 2, 3, 5] * 4, dtype=np.float32)
    diag_a = np.array([4, 16, 16, 64] * 4, dtype=np.float32)
    Y = np.zeros((d * 3, d), dtype=np.float32)
    a_item = np.zeros(d * 3, dtype=np.float32)
    for j in range(d):
        for c, (a_c, f_c) in enumerate(_EXACT_GROUPS):
            Y[j * 3 + c, j] = rng.choice([-1.0, 1.0]) * mag[j] * f_c
            a_item[j * 3 + c] = a_c
    G = np.diag(diag_a - mag * mag - 1.0).astype(np.float32)
    rows = [[]]
    for _ in range(20):                                          # one item of every column, any group, in a random order
        rows.append(rng.permutation([j * 3 + int(rng.integers(3)) for j in range(d)]).tolist())
    conf = [a_item[np.asarray(e, dtype=np.int64)] for e in rows]
    return Y, G, rows, conf, np.ones(len(rows), dtype=np.float32)


def exact_block_case():
    """als_block_cases.exact_case (d = 32, B = 16, reg = 1) with weights: the items of group c carry a_e = a_c and have their
    entries scaled by f_c, a_c f_c^2 = 1, so every block system keeps its power-of-4 diagonal; the blocks still couple
    through p_e and w_e = a_e p_e - (1 + a_e).  Returns (Y, G, rows, conf, reg_rows, X0)."""
    Y, G, rows, X0 = BC.exact_case()
    Y = Y.copy()
    per = Y.shape[0] // 3
    a_item = np.zeros(Y.shape[0], dtype=np.float32)
    for c, (a_c, f_c) in enumerate(_EXACT_GROUPS):
        Y[c * per:(c + 1) * per] *= np.float32(f_c)
        a_item[c * per:(c + 1) * per] = a_c
    conf = [a_item[np.asarray(e, dtype=np.int64)] for e in rows]
    return Y, G, rows, conf, np.ones(len(rows), dtype=np.float32), X0
