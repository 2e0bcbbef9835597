"""Without a GPU: the NumPy restatement of the lazy Adam row update (tests/lazy_adam_emulation.py) against torch.optim.SparseAdam
on the CPU, and the size queries and argument validation of mi_lazy_adam_rows_f32, mi_pinsage_project_bwd_lazy_f32 and
mi_pinsage_text_bwd_lazy_f32 (nothing is enqueued by any call here)."""
import ctypes

import numpy as np
import pytest
import torch as t

import lazy_adam_emulation as LE

R, W, STEPS, LR = 97, 20, 40, 0.05
BETAS, EPS = (0.9, 0.999), 1e-8


def test_emulation_against_torch_sparse_adam():
    """40 steps over random subsets of a 97 x 20 table, gradient scales 1e-6 .. 1e2, one referenced all-zero row per step.
    exp_avg / exp_avg_sq: equal bits on every step.  p: |delta| <= S * 2^-23 * (max|p| + 4 * max|q * ss|) after S steps —
    torch's CPU sqrt is not correctly rounded everywhere, which moves p by an ulp of the update now and then."""
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal((R, W)).astype(np.float32)
    param = t.nn.Parameter(t.from_numpy(p0.copy()))
    opt = t.optim.SparseAdam([param], lr=LR, betas=BETAS, eps=EPS)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    never = np.ones(R, dtype=bool)
    max_upd = 0.0
    for step in range(1, STEPS + 1):
        n = int(rng.integers(1, R // 2))
        rows = rng.choice(R, n, replace=False)
        scale = np.float32(10.0 ** rng.uniform(-6, 2))
        g = (rng.standard_normal((n, W)) * scale).astype(np.float32)
        g[0] = 0.0                                                    # referenced, gradient exactly zero
        was = (p[rows[0]].copy(), m[rows[0]].copy())
        param.grad = t.sparse_coo_tensor(t.from_numpy(rows)[None], t.from_numpy(g), (R, W))
        opt.step()
        max_upd = max(max_upd, LE.update_rows(p, m, v, rows, g, LR, *BETAS, EPS, step))
        never[rows] = False
        st = opt.state[param]
        assert np.array_equal(st["exp_avg"].numpy().view(np.int32), m.view(np.int32)), step
        assert np.array_equal(st["exp_avg_sq"].numpy().view(np.int32), v.view(np.int32)), step
        if np.any(was[1] != 0):
            assert not np.array_equal(p[rows[0]], was[0])             # a zero gradient with live moments still moves the row
            assert not np.array_equal(m[rows[0]], was[1])
        bound = step * 2.0 ** -23 * (float(np.abs(p).max()) + 4 * max_upd)
        err = float(np.abs(param.detach().numpy().astype(np.float64) - p.astype(np.float64)).max())
        assert err <= bound, (step, err, bound)
    assert st["step"] == STEPS
    if never.any():                                                   # rows nobody referenced keep every bit
        assert np.array_equal(p[never], p0[never]) and not m[never].any() and not v[never].any()


def test_constants_are_the_host_side_doubles():
    c1, c2, e, ss = LE.constants(0.05, 0.9, 0.999, 1e-8, 3)
    assert c1 == np.float32(1.0 - 0.9) and c2 == np.float32(1.0 - 0.999) and e == np.float32(1e-8)
    assert ss == np.float32(-(0.05 * (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3))) and ss.dtype == np.float32


# ---- the C entries without a GPU -----------------------------------------------------------------------------------------------
def _lazy(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, step=1):
    from laplace_amd import _lib
    z = _lib.LazyAdam()
    z.lr, z.beta1, z.beta2, z.eps, z.step = lr, b1, b2, eps, step
    return z


def test_sizes_and_rows_entry_validation():
    from laplace_amd import _lib
    L = _lib.lib()
    assert L.mi_lazy_adam_sizeof(0) == ctypes.sizeof(_lib.LazyAdam) == 40
    assert L.mi_lazy_adam_sizeof(1) == ctypes.sizeof(_lib.ItemProjectorMoments)
    assert L.mi_lazy_adam_sizeof(2) == -1
    A = 1 << 20                      # an aligned address that is never dereferenced: every call below returns before a launch
    lz = ctypes.byref(_lazy())
    call = L.mi_lazy_adam_rows_f32
    BAD, UNS = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_UNSUPPORTED
    assert call(100, 16, A, A, A, 5, A, A, 16, None, None) == BAD                      # no hyper-parameters
    assert call(100, 16, A, A, A, 5, A, A, 16, ctypes.byref(_lazy(step=0)), None) == BAD
    assert call(100, 16, A, A, A, 5, A, A, 16, ctypes.byref(_lazy(b1=1.0)), None) == BAD
    assert call(100, 16, A, A, A, 5, A, A, 16, ctypes.byref(_lazy(lr=-1.0)), None) == BAD
    for width in (0, 2, 18, 516):
        assert call(100, width, A, A, A, 5, A, A, 520, lz, None) == UNS, width
    assert call(100, 16, None, A, A, 5, A, A, 16, lz, None) == BAD
    assert call(100, 16, A, A + 4, A, 5, A, A, 16, lz, None) == BAD                    # misaligned moment
    assert call(100, 16, A, A, A, -1, A, A, 16, lz, None) == BAD
    assert call(100, 16, A, A, A, 101, A, A, 16, lz, None) == BAD                      # more distinct ids than rows
    assert call(100, 16, A, A, A, 5, None, A, 16, lz, None) == BAD
    assert call(100, 16, A, A, A, 5, A, A, 12, lz, None) == BAD                        # ldg < width
    assert call(100, 16, A, A, A, 5, A, A, 18, lz, None) == BAD                        # ldg % 4
    assert call(0, 16, A, A, A, 0, A, A, 16, lz, None) == BAD
    assert call(100, 16, A, A, A, 0, None, None, 16, lz, None) == 0                    # nothing to do: nothing enqueued


def _projector(hidden=16, n_items=50, use_id=True):
    from laplace_amd import _lib
    A = 1 << 20
    d = _lib.ItemProjector()
    d.hidden, d.n_cols, d.n_items, d.x = hidden, 1, n_items, A
    d.tables[0], d.table_rows[0] = A, 3
    d.id_table = A if use_id else None
    gd = _lib.ItemProjectorGrads()
    gd.g_tables[0], gd.g_id_table = A, (A if use_id else None)
    return d, gd


def test_project_bwd_lazy_validation():
    from laplace_amd import _lib
    L = _lib.lib()
    A = 1 << 20
    BAD, WS = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    call = L.mi_pinsage_project_bwd_lazy_f32
    d, gd = _projector()
    need = L.mi_pinsage_project_bwd_workspace_bytes(ctypes.byref(d), 40)      # the lazy entry takes the same workspace
    assert need > 0
    lz = ctypes.byref(_lazy())
    mo = _lib.ItemProjectorMoments()
    mo.m_id_table = A                                                           # half a pair
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 16, A, need, None) == BAD
    mo.v_id_table = A + 8                                                       # misaligned
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 16, A, need, None) == BAD
    mo.v_id_table = A
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), None, 40, A, A, 16, A, need, None) == BAD   # lazy slot, no hyper-parameters
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), ctypes.byref(_lazy(step=0)), 40, A, A, 16, A, need, None) == BAD
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 16, A, need - 1, None) == WS
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 16, None, need, None) == WS
    assert call(None, ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 16, A, need, None) == BAD
    d2, gd2 = _projector(use_id=False)
    assert call(ctypes.byref(d2), ctypes.byref(gd2), ctypes.byref(mo), lz, 40, A, A, 16, A, need, None) == BAD   # moments for no id table
    d.hidden = 132
    assert call(ctypes.byref(d), ctypes.byref(gd), ctypes.byref(mo), lz, 40, A, A, 132, A, need, None) == _lib.MI_ERR_UNSUPPORTED


def test_text_bwd_lazy_validation():
    from laplace_amd import _lib
    L = _lib.lib()
    A = 1 << 20
    BAD, WS = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_WORKSPACE
    call = L.mi_pinsage_text_bwd_lazy_f32
    d = _lib.TextColumns()
    d.width, d.n_text, d.n_items = 16, 2, 50
    for c in range(2):
        d.ptr[c], d.tok[c], d.tables[c], d.vocab[c] = A, A, A, 64
    need = L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(d), 40, 500)     # the lazy entry takes the same workspace
    assert need > 0
    gt, mt, vt = _lib.TextGradTables(), _lib.TextGradTables(), _lib.TextGradTables()
    gt[0] = gt[1] = A
    lz = ctypes.byref(_lazy())
    args = (40, A, A, 16, 500, A, need, None)
    mt[0] = A                                                                   # half a pair
    assert call(ctypes.byref(d), gt, mt, vt, lz, *args) == BAD
    vt[0] = A
    assert call(ctypes.byref(d), gt, mt, None, lz, *args) == BAD               # one of the two arrays missing
    assert call(ctypes.byref(d), gt, mt, vt, None, *args) == BAD
    assert call(ctypes.byref(d), gt, mt, vt, ctypes.byref(_lazy(b2=-0.1)), *args) == BAD
    vt[0] = A + 4
    assert call(ctypes.byref(d), gt, mt, vt, lz, *args) == BAD
    vt[0] = A
    assert call(ctypes.byref(d), gt, mt, vt, lz, 40, A, A, 16, 500, A, need - 1, None) == WS
    assert call(ctypes.byref(d), gt, mt, vt, lz, 40, A, A, 16, 2 ** 31, A, need, None) == _lib.MI_ERR_TOO_LARGE
    d.width = 520
    assert call(ctypes.byref(d), gt, mt, vt, lz, *args) == _lib.MI_ERR_UNSUPPORTED
