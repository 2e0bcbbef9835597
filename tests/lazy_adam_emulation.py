"""CPU emulation, in NumPy float32, of the row update of mi_lazy_adam_rows_f32, mi_pinsage_project_bwd_lazy_f32 and
mi_pinsage_text_bwd_lazy_f32 (csrc/lazy_adam.hpp) — torch.optim.SparseAdam's arithmetic, one float32 rounding per operation:

    d  = g - m            m' = m + d * c1         c1 = float32(1 - beta1)
    s  = g*g - v          v' = v + s * c2         c2 = float32(1 - beta2)
    q  = m' / (sqrt(v') + float32(eps))
    p' = p + q * ss       ss = float32(-lr * sqrt(1 - beta2^t) / (1 - beta1^t))    in double, t = step (from 1)

NumPy's float32 +, -, *, / and sqrt are correctly rounded and never contracted, as the kernels' chain is (plain operators with
contraction switched off, and the correctly rounded sqrtf and division: csrc/lazy_adam.hpp).  The GPU tests compare the kernels' tables with it bit for bit."""
import math

import numpy as np

F = np.float32


def constants(lr, beta1, beta2, eps, step):
    """(c1, c2, eps, ss) as float32; the step size in double first, as the host code derives it."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return F(1.0 - beta1), F(1.0 - beta2), F(eps), F(-(lr * math.sqrt(bc2) / bc1))


def update_rows(p, m, v, rows, g, lr, beta1, beta2, eps, step):
    """In place on float32 [R, W] arrays p, m, v: the rows `rows` (distinct) with gradient rows g [len(rows), W]; every other row
    keeps its bits.  Returns max |q * ss| of the call (0 for no rows) for error bounds."""
    rows = np.asarray(rows, dtype=np.int64)
    assert len(np.unique(rows)) == len(rows) and p.dtype == m.dtype == v.dtype == F
    if len(rows) == 0:
        return 0.0
    c1, c2, e, ss = constants(lr, beta1, beta2, eps, step)
    g = np.asarray(g, dtype=F)
    m0, v0 = m[rows], v[rows]
    m1 = m0 + (g - m0) * c1
    v1 = v0 + (g * g - v0) * c2
    q = m1 / (np.sqrt(v1) + e)
    upd = q * ss
    p[rows] = p[rows] + upd
    m[rows] = m1
    v[rows] = v1
    assert m1.dtype == v1.dtype == upd.dtype == F
    return float(np.abs(upd).max())


def update_from_sums(p, m, v, sums, slot, lr, beta1, beta2, eps, step):
    """update_rows over the summed rows segsum_emulation.segmented_sum returned for table `slot` (keys slot * SLOT + row)."""
    from segsum_emulation import SLOT
    keys = sorted(k for k in sums if k // SLOT == slot)
    rows = np.array([k % SLOT for k in keys], dtype=np.int64)
    g = np.stack([sums[k] for k in keys]) if keys else np.zeros((0, p.shape[1]), dtype=F)
    return update_rows(p, m, v, rows, g, lr, beta1, beta2, eps, step), rows
