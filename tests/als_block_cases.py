"""Inputs shared by tests/test_als_block_cpu.py and tests/test_gpu_als_block.py (numpy only): the (d, B) problems of the GPU
test with their float64 and float32 references, computed once per process, and the exact case."""
import numpy as np

import als_block_emulation as BE
from laplace_amd import ops

ALPHA, REG = 1.5, 0.75
N_COLS, N_ROWS = 300, 40
DIMS = (16, 40, 64, 128, 256)
BLOCKS = (16, 32, 64)
STARTS = ((True, 1), (False, 1), (True, 3), (False, 3))   # (from zero, sweeps)
LONG_ROW = 7


class Problem:
    """One (d, B): rows of lengths 0, 1, 3, B - 1, B + 1, 33, 70, one longer than ops.als_block_chunk(d, B) (the only constant
    the kernel exposes), and random short ones up to N_ROWS, over a column slice (ldy = d + 8) of a wider table whose rows
    share an offset (G, S and b are then dominated by one direction, as trained factors are); a warm start X0."""

    def __init__(self, d, B):
        rng = np.random.default_rng(1000 * d + B)
        self.d, self.B, self.chunk = d, B, ops.als_block_chunk(d, B)
        lens = [0, 1, 3, B - 1, B + 1, 33, 70, self.chunk + 5]
        assert lens[LONG_ROW] > self.chunk > 0
        lens += rng.integers(1, 40, N_ROWS - len(lens)).tolist()
        self.rows = [rng.integers(0, N_COLS, n).tolist() for n in lens]
        self.wide = (0.25 + rng.standard_normal((N_COLS, d + 8)) * 0.2).astype(np.float32)
        self.Y = self.wide[:, 4:4 + d]
        G = self.Y.astype(np.float64).T @ self.Y.astype(np.float64)
        self.G = BE.sym_lower(G.astype(np.float32))
        self.X0 = (rng.standard_normal((N_ROWS, d)) * 0.1).astype(np.float32)
        self._refs = {}

    def refs(self, from_zero, sweeps):
        """(X64, X32, tol): the rule in float64, the float32 reference, and 8 * max_r ||x_f32ref - x_64||_2."""
        key = (from_zero, sweeps)
        if key not in self._refs:
            X64 = np.zeros((N_ROWS, self.d))
            X32 = np.zeros((N_ROWS, self.d), dtype=np.float32)
            for r, e in enumerate(self.rows):
                x0 = None if from_zero else self.X0[r]
                X64[r] = BE.block_sweep64(e, self.Y, self.G, ALPHA, REG, x0, self.B, sweeps)
                X32[r] = BE.block_sweep_f32(e, self.Y, self.G, ALPHA, REG, x0, self.B, sweeps)
            tol = 8.0 * np.linalg.norm(X32.astype(np.float64) - X64, axis=1).max()
            self._refs[key] = (X64, X32, tol)
        return self._refs[key]


_PROBLEMS = {}


def problem(d, B):
    if (d, B) not in _PROBLEMS:
        _PROBLEMS[(d, B)] = Problem(d, B)
    return _PROBLEMS[(d, B)]


def exact_case():
    """d = 32, B = 16, alpha = reg = 1.  Every factor row has one non-zero in each block (a small integer, signed), the entries
    of a user row have theirs in different columns, G is diagonal and G[j][j] = H_j - m_j^2 - 1 with H_j a power of 4: every
    block system is diagonal with power-of-4 pivots, and every operation of the rule — the square roots and their
    reciprocals included — is exact in float32.  The blocks still couple through p_e.  Returns (Y, G, rows, X0), X0 a warm
    start of quarters."""
    d, B, per = 32, 16, 3
    rng = np.random.default_rng(7)
    mag = np.array([1, 2, 3, 2] * 8, dtype=np.float32)            # |entry| of the items of column j
    hdiag = np.array([4, 16, 16, 64] * 8, dtype=np.float32)
    # item (j, c): columns j (block 0) and 16 + sigma_c(j) (block 1), sigma_c a permutation: the items of one c never share a column
    sig = [rng.permutation(B) for _ in range(per)]
    Y = np.zeros((B * per, d), dtype=np.float32)
    for c in range(per):
        for j in range(B):
            Y[c * B + j, j] = rng.choice([-1.0, 1.0]) * mag[j]
            k = B + sig[c][j]
            Y[c * B + j, k] = rng.choice([-1.0, 1.0]) * mag[k]
    G = np.diag(hdiag - mag * mag - 1.0).astype(np.float32)
    rows = [[]]
    for _ in range(12):                                           # a subset of the items of one c, in a random order
        c = int(rng.integers(per))
        rows.append((c * B + rng.permutation(B)[:int(rng.integers(1, B + 1))]).tolist())
    X0 = (rng.integers(-4, 5, (len(rows), d)) / 4.0).astype(np.float32)
    for r, e in enumerate(rows):                                  # a column no entry touches has H_j = G_jj + 1, no power of 4:
        X0[r, ~(Y[e] != 0).any(axis=0)] = 0.0                     # it starts, and stays, at zero
    return Y, G, rows, X0
