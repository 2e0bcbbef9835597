"""No GPU: the popularity-weighted negative table (properties of ops.negative_table), the draw rule on the numpy mirror
(frequencies follow the table), and the argument checks of the trainer, the ops and the two C entries."""
import os
import sys

import numpy as np
import pytest
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import neg_sampling_emulation as E  # noqa: E402

SIZES, POWERS = (64, 1000), (0.0, 0.75, 1.0)


def _zipf_degrees(n):
    """floor(2000 / i), i = 1..n, with n / 8 items zeroed."""
    deg = np.floor(2000.0 / np.arange(1, n + 1)).astype(np.int64)
    deg[np.random.default_rng(0).permutation(n)[: n // 8]] = 0
    return deg


def _table(n, power):
    from laplace_amd import ops
    deg = _zipf_degrees(n)
    return deg, ops.negative_table(t.from_numpy(deg), power, device="cpu")


# ---------------------------------------------------------------------------- 1: table properties
@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("n", SIZES)
def test_table_properties(n, power):
    deg, tab = _table(n, power)
    assert tab.n_items == n and tab.power == power
    assert tab.cum.dtype == t.int32 and tuple(tab.cum.shape) == (n,)
    assert tab.logq.dtype == t.float32 and tuple(tab.logq.shape) == (n,)
    cum = E.cum_u32(tab).astype(np.int64)
    q = np.diff(cum, prepend=0)
    assert (q >= 0).all()                                          # cum is non-decreasing
    assert ((q == 0) == (deg == 0)).all()
    assert tab.total == int(cum[-1]) and 0 < tab.total < 2 ** 32
    w = np.where(deg > 0, np.where(deg > 0, deg, 1).astype(np.float64) ** power, 0.0)
    p = w / w.sum()
    err = np.abs(q / tab.total - p).max()
    print(f"n={n} power={power}: total {tab.total}, max |q/total - w/S| {err:.3e}, bound {(n + 1) / (2 ** 31 - n):.3e}")
    assert err <= (n + 1) / (2 ** 31 - n)
    has = deg > 0
    if power == 0.0:
        assert len(set(q[has].tolist())) == 1                      # equal weights to every item with a degree
    if power == 1.0:                                               # weights ∝ degree (to the floor's 1 in 2^31 * p)
        ratio = q[has] / deg[has]
        assert ratio.max() - ratio.min() <= 1.0 + 1e-9
    logq = tab.logq.numpy()
    want = np.log(np.maximum(q, 1) / tab.total)
    assert np.isfinite(logq).all()
    assert (logq == want.astype(np.float32)).all()
    assert (np.abs(logq.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want)).all()


def test_table_refuses_what_it_cannot_draw_from():
    from laplace_amd import ops
    with pytest.raises(ValueError):
        ops.negative_table(t.zeros(10, dtype=t.int64), 0.75, device="cpu")      # all-zero degrees
    with pytest.raises(ValueError):
        ops.negative_table_from_counts(np.zeros(5, dtype=np.int64), "cpu")
    with pytest.raises(ValueError):
        ops.negative_table_from_counts(np.array([1, -1, 3]), "cpu")
    with pytest.raises(ValueError):
        ops.negative_table_from_counts(np.array([2 ** 31, 2 ** 31]), "cpu")     # total = 2^32
    with pytest.raises(ValueError):
        ops.negative_table_from_counts(np.array([0.5, 1.0]), "cpu")
    with pytest.raises(ValueError):
        ops.negative_table(t.tensor([3, -1]), 0.75, device="cpu")
    for power in (-0.1, 1.5, None, "1", True):
        with pytest.raises(ValueError):
            ops.negative_table(t.tensor([3, 1]), power, device="cpu")
    tab = ops.negative_table_from_counts(np.array([0, 0, 5, 0, 1, 0, 0]), "cpu")
    assert tab.total == 6 and tab.n_items == 7 and tab.power is None
    assert E.cum_u32(tab).tolist() == [0, 0, 5, 5, 6, 6, 6]
    assert np.allclose(tab.logq.numpy(), np.log(np.array([1, 1, 5, 1, 1, 1, 1]) / 6.0))
    top = ops.negative_table_from_counts(np.array([2 ** 31, 2 ** 31 - 1]), "cpu")   # the words above 2^31 keep their bits
    assert top.total == 2 ** 32 - 1 and E.cum_u32(top).tolist() == [2 ** 31, 2 ** 32 - 1]


# ---------------------------------------------------------------------------- 2: the draws follow the table
@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("n", SIZES)
def test_mirror_draws_follow_the_table(n, power):
    """A condition on the RULE (counter -> r % total -> smallest i with cum[i] > r), checked on the mirror the GPU tests
    hold the kernel to bit for bit.  Measured here, largest |freq - p| / sqrt(p (1 - p) / N) over the six cases: 3.58."""
    deg, tab = _table(n, power)
    cum = E.cum_u32(tab)
    N = 2 ** 16 if n == 64 else 2 ** 18
    cand = E.draw(cum, np.arange(N), 0, 0, seed=0xBEEF0000CAFE, step=7)
    assert cand.min() >= 0 and cand.max() < n
    freq = np.bincount(cand, minlength=n) / N
    q = np.diff(cum.astype(np.int64), prepend=0)
    p = q / tab.total
    assert (freq[q == 0] == 0).all()                               # no zero-weight item is ever drawn
    has = q > 0
    ratio = np.abs(freq[has] - p[has]) / np.sqrt(p[has] * (1.0 - p[has]) / N)
    print(f"n={n} power={power}: largest deviation {ratio.max():.2f} standard errors")
    assert (ratio <= 5.0).all()


def test_mirror_rejects_user_items_and_keeps_the_edge_stream():
    g = np.random.default_rng(1)
    U, I = 30, 12
    keys = np.sort(g.permutation(U * I)[:150])
    rows, col = keys // I, keys % I
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=U))])
    from laplace_amd import ops
    tab = ops.negative_table(t.from_numpy(np.bincount(col, minlength=I)), 0.75, device="cpu")
    cum = E.cum_u32(tab)
    u1, p1, n1 = E.sample(rowptr, col, 256, 1, cum, seed=9, step=3)
    u4, p4, n4 = E.sample(rowptr, col, 256, 4, cum, seed=9, step=3)
    assert (u1 == u4).all() and (p1 == p4).all() and (n1[:, 0] == n4[:, 0]).all()
    held = set((rows * I + col).tolist())
    assert all(int(u) * I + int(p) in held for u, p in zip(u4, p4))
    assert not any(int(u) * I + int(x) in held for u, row in zip(u4, n4) for x in row)


# ---------------------------------------------------------------------------- 3: argument checks
def _tiny_model():
    from laplace_amd.model.lightgcn import LightGCN
    return LightGCN(4, 5, 8, 1)


@pytest.mark.parametrize("kw", [
    dict(negatives="zipf"), dict(negatives=None), dict(negatives=True),
    dict(neg_power=-0.01), dict(neg_power=1.01), dict(neg_power=None), dict(neg_power="0.75"),
    dict(negatives="popularity", neg_power=2.0),
    dict(logq_correction=True), dict(logq_correction=True, objective="bpr", n_neg=4),
    dict(logq_correction=True, objective="reference", negatives="popularity"),
    dict(negatives="popularity", reference_sampler_quirks=True),
    dict(negatives="popularity", objective="softmax", n_neg=4, neg_range=4),
    dict(negatives="popularity", neg_range=6)])
def test_trainer_refuses_bad_negative_options_before_the_gpu(kw):
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(ValueError):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(negatives="uniform"), dict(negatives="popularity", neg_range=5),
                                dict(negatives="popularity", objective="softmax", n_neg=4, logq_correction=False),
                                dict(objective="softmax", logq_correction=True), dict(neg_power=0), dict(neg_power=1)])
def test_trainer_accepts_the_valid_options_up_to_the_device_check(kw):
    """In range, the constructor gets as far as the model's device: no CPU fallback."""
    from laplace_amd.trainer import LightGCNTrainer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LightGCNTrainer(_tiny_model(), None, None, lr=1e-3, Lambda=1e-6, batch_size=4, **kw)


def test_ops_refuse_bad_tables_and_logq():
    from laplace_amd import ops
    from laplace_amd._lib import MiError
    from laplace_amd.utils.metrics_lightgcn import ranking_loss
    tab = ops.negative_table_from_counts(np.array([1, 2, 3, 4, 5]), "cpu")
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(None, None, 4, 6, 0, 0, table=tab)                  # neg_range != n_items
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(None, None, 4, 5, 0, 0, table=tab, quirk=True)
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(None, None, 4, 5, 0, 0, table=tab, no_self_loops=True)
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(None, None, 4, 5, 0, 0, table=tab, n_neg=17)
    with pytest.raises(ValueError):
        ops.sample_bpr_batch(None, None, 0, 5, 0, 0, table=tab)
    with pytest.raises(TypeError):
        ops.sample_bpr_batch(None, None, 4, 5, 0, 0, table=tab.cum)
    u, p, n = t.zeros(4, dtype=t.int64), t.zeros(4, dtype=t.int64), t.zeros(4, 2, dtype=t.int64)
    emb = t.zeros(9, 8)
    for objective in ("reference", "bpr"):
        with pytest.raises(ValueError):
            ops.rank_loss_fwd_bwd(u, p, n, emb, emb, 4, 1e-6, objective=objective, logq=t.zeros(5))
    with pytest.raises(MiError):   # in range: the device check is next, no CPU fallback
        ops.rank_loss_fwd_bwd(u, p, n, emb, emb, 4, 1e-6, objective="softmax", logq=t.zeros(5))
    blocks = [t.zeros(4, 8)] * 4 + [t.zeros(4, 2, 8)] * 2
    with pytest.raises(ValueError):
        ranking_loss(*blocks, 1e-6, objective="bpr", logq=(t.zeros(4), t.zeros(4, 2)))
    with pytest.raises(ValueError):
        ranking_loss(*blocks, 1e-6, objective="softmax", logq=(t.zeros(4), t.zeros(4, 3)))
    with pytest.raises(ValueError):
        ranking_loss(*blocks, 1e-6, objective="softmax", logq=(t.zeros(5), t.zeros(4, 2)))


def test_c_entries_check_their_arguments_before_any_launch():
    import ctypes
    from laplace_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, BAD_ARG, TOO_LARGE = _lib.MI_ERR_UNSUPPORTED, _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_TOO_LARGE
    assert L.mi_abi_version() == 14
    buf = (ctypes.c_int64 * 64)()
    ok = ctypes.addressof(buf)

    def pop(batch=8, n_neg=3, nnz=10, rowptr=ok, col=ok, roe=ok, n_items=5, cum=ok, in_order=0, users=ok, pos=ok, neg=ok):
        return L.mi_sample_bpr_batch_pop(batch, n_neg, nnz, rowptr, col, roe, n_items, cum, in_order, 0, 0, users, pos,
                                         neg, None)
    assert pop(n_neg=17) == UNSUPPORTED
    for kw in (dict(n_neg=0), dict(n_neg=-1), dict(batch=0), dict(batch=-1), dict(nnz=0), dict(n_items=0),
               dict(rowptr=None), dict(col=None), dict(roe=None), dict(cum=None), dict(users=None), dict(pos=None),
               dict(neg=None), dict(cum=ok + 2), dict(col=ok + 1), dict(neg=ok + 4), dict(users=ok + 4),
               dict(batch=11, in_order=1)):
        assert pop(**kw) == BAD_ARG, kw
    assert pop(n_items=2 ** 31) == TOO_LARGE and pop(nnz=2 ** 31 - 1) == TOO_LARGE

    def rank(objective, logq, g_final=None, reg_w=None, n_neg=4, d=64):
        return L.mi_rank_loss_fwd_bwd_lq_f32(8, n_neg, objective, d, 4, None, None, None, None, d, None, d, 1e-6, 1.0, 1.0,
                                             None, g_final, d, reg_w, None, logq, None, 0, None)
    for objective in (0, 1):
        assert rank(objective, ok) == UNSUPPORTED                  # a logq with another objective
        assert rank(objective, None) == BAD_ARG                    # without: the null pointers are next
    assert rank(2, ok, g_final=ok, reg_w=ok) == BAD_ARG and rank(2, None) == BAD_ARG
    assert rank(2, ok, g_final=None, reg_w=ok) == UNSUPPORTED      # the one form that accumulates with float atomics
    assert rank(2, ok, n_neg=17) == UNSUPPORTED and rank(3, ok) == UNSUPPORTED
