"""Inputs shared by tests/test_als_hub_cpu.py and tests/test_gpu_als_hub.py (numpy only): als_block_cases.Problem's table, G
and rows with the rows the hub thresholds need, their float64 and float32 block references (computed once per process), and
the weighted twin."""
import numpy as np

import als_block_cases as BC
import als_block_emulation as BE
import als_weighted_cases as WC
import als_weighted_emulation as WE
from laplace_amd import ops

ALPHA, REG, N_COLS = BC.ALPHA, BC.REG, BC.N_COLS
THRESHOLDS = (4, 64)
SHAPES = ((16, 16), (40, 16), (64, 32), (128, 32), (256, 16), (256, 64))
MULTI_CHUNK = ((16, 16), (256, 16))                    # the shapes that carry rows of several chunks of L_h entries
W_SHAPES = WC.BLOCK_SHAPES                             # (40, 16), (128, 32), (256, 64)
ZERO_COL = N_COLS                                      # an all-zero factor row behind the table's N_COLS rows


class Problem:
    """One (d, B).  Rows: als_block_cases.Problem's 40 (lengths 0, 1, 3, B - 1, B + 1, 33, 70, chunk + 5 and random ones below
    40), then T and T + 1 for both thresholds (4, 5, 64, 65), and with `multi` the rows L_h - 1, L_h, L_h + 1, 2 L_h + 3
    (L_h = ops.als_block_hub_chunk(d)) and the L_h row again with a zero factor row as entry L_h + 1.  The table is the base
    problem's (a column slice, ldy = d + 8, rows sharing an offset) with one zero row appended; nothing of the base problem is
    written."""

    def __init__(self, d, B, multi):
        base = BC.problem(d, B)
        rng = np.random.default_rng(5000 * d + B)
        self.d, self.B, self.L = d, B, ops.als_block_hub_chunk(d)
        assert self.L > 0
        self.rows = [list(e) for e in base.rows]
        self.named = {}
        for n in (4, 5, 64, 65):
            self.named[n] = len(self.rows)
            self.rows.append(rng.integers(0, N_COLS, n).tolist())
        self.multi = []
        if multi:
            L = self.L
            for n in (L - 1, L, L + 1, 2 * L + 3):
                self.multi.append(len(self.rows))
                self.rows.append(rng.integers(0, N_COLS, n).tolist())
            self.boundary = (self.multi[1], len(self.rows))          # the L_h row and its twin with a zero entry behind it
            self.rows.append(self.rows[self.multi[1]] + [ZERO_COL])
        self.n_rows = len(self.rows)
        self.wide = np.concatenate([base.wide, np.zeros((1, d + 8), dtype=np.float32)])
        self.Y = self.wide[:, 4:4 + d]
        self.G = base.G
        self.X0 = np.concatenate([base.X0, (rng.standard_normal((self.n_rows - BC.N_ROWS, d)) * 0.1).astype(np.float32)])
        if multi:
            self.X0[self.boundary[1]] = self.X0[self.boundary[0]]
        self._refs = {}

    def sweep64(self, r, x0, sweeps):
        return BE.block_sweep64(self.rows[r], self.Y, self.G, ALPHA, REG, x0, self.B, sweeps)

    def sweep32(self, r, x0, sweeps):
        return BE.block_sweep_f32(self.rows[r], self.Y, self.G, ALPHA, REG, x0, self.B, sweeps)

    def refs(self, from_zero, sweeps):
        """(X64, err32): the block rule in float64 and ||x_f32ref - x_64||_2 per row, x_f32ref the committed block_sweep_f32."""
        key = (from_zero, sweeps)
        if key not in self._refs:
            X64 = np.zeros((self.n_rows, self.d))
            err = np.zeros(self.n_rows)
            for r in range(self.n_rows):
                x0 = None if from_zero else self.X0[r]
                X64[r] = self.sweep64(r, x0, sweeps)
                err[r] = np.linalg.norm(self.sweep32(r, x0, sweeps).astype(np.float64) - X64[r])
            self._refs[key] = (X64, err)
        return self._refs[key]

    def hub_rows(self, threshold):
        return [r for r, e in enumerate(self.rows) if len(e) > threshold]


class WeightedProblem(Problem):
    """The same rows with a confidence per entry (log-uniform in [0.1, 30]) and a regulariser per row (uniform in [0.5, 5])."""

    def __init__(self, d, B, multi):
        super().__init__(d, B, multi)
        rng = np.random.default_rng(6000 * d + B)
        self.conf = [np.exp(rng.uniform(np.log(0.1), np.log(30.0), len(e))).astype(np.float32) for e in self.rows]
        if multi:                                                     # the twin's entries carry the L_h row's confidences
            one, two = self.boundary
            self.conf[two] = np.concatenate([self.conf[one], self.conf[two][-1:]])
        self.reg_rows = rng.uniform(0.5, 5.0, self.n_rows).astype(np.float32)
        self.reg_mode = True          # False: reg_rows null, the scalar REG for every row
        self._refs_w = {}

    def reg_of(self, r):
        return self.reg_rows[r] if self.reg_mode else np.float32(REG)

    def sweep64(self, r, x0, sweeps):
        return WE.block_sweep64(self.rows[r], self.conf[r], self.Y, self.G, self.reg_of(r), x0, self.B, sweeps)

    def sweep32(self, r, x0, sweeps):
        return WE.block_sweep_f32(self.rows[r], self.conf[r], self.Y, self.G, self.reg_of(r), x0, self.B, sweeps)

    def refs_w(self, from_zero, sweeps, with_reg_rows):
        key = (from_zero, sweeps, with_reg_rows)
        if key not in self._refs_w:
            self.reg_mode, self._refs = with_reg_rows, {}
            self._refs_w[key] = self.refs(from_zero, sweeps)
        return self._refs_w[key]


_PROBLEMS = {}


def problem(d, B):
    if (d, B) not in _PROBLEMS:
        _PROBLEMS[(d, B)] = Problem(d, B, (d, B) in MULTI_CHUNK)
    return _PROBLEMS[(d, B)]


def weighted_problem(d, B):
    if ("w", d, B) not in _PROBLEMS:
        _PROBLEMS[("w", d, B)] = WeightedProblem(d, B, d == 256)
    return _PROBLEMS[("w", d, B)]


def csr_arrays(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ptr, idx
