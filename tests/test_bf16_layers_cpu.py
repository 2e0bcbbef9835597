"""bf16 layer tables, without a device: the mirror of the rule (tests/bf16_layers_emulation.py) against the float64 reference on
exactly the inputs the GPU tests use, inside the derived bounds — which shows on the CPU that the bounds are right for those
inputs — the order of additions of the mirror's read-out, and the refusals that need no GPU."""
import numpy as np
import pytest
import torch as t

import bf16_layers_emulation as E

F = np.float32


@pytest.fixture(scope="module")
def graph():
    return E.adjacency()


@pytest.mark.parametrize("chunk", [None, 8])
@pytest.mark.parametrize("d", E.WIDTHS)
def test_mirror_stays_inside_the_derived_bounds(graph, d, chunk):
    rowptr, col, val = graph
    x, addend = E.operand(d)
    exact, absum, n = E.spmm_f64(rowptr, col, val, x)
    acc = E.spmm_mirror(rowptr, col, val, x, chunk)
    assert set(n.tolist()) >= {0, 1, 7, 8, 9, 100, E.N_COLS}
    # S without Y (scale and addend), Y alone, S beside Y
    _, s = E.epilogue_mirror(acc, False, addend, 0.25)
    err = np.abs(s.astype(np.float64) - 0.25 * (addend.astype(np.float64) + exact))
    assert (err <= E.bound_s(n, absum, exact, addend, 0.25)).all()
    y, s2 = E.epilogue_mirror(acc, True, addend, -2.0)
    assert (np.abs(y.astype(np.float64) - exact) <= E.bound_y(n, absum, exact)).all()
    err2 = np.abs(s2.astype(np.float64) - (-2.0) * (addend.astype(np.float64) + exact))
    assert (err2 <= E.bound_s_with_y(n, absum, exact, addend, -2.0)).all()
    # the bounds are not vacuous: a bf16 rounding of the sum does not fit the f32 bound
    big = np.abs(exact) > 0.5
    assert (np.abs(E.rn(acc) - exact)[big] > E.bound_s(n, absum, exact, None, 1.0)[big]).any()


def test_mirror_of_the_row_list_is_the_dense_mirror_on_the_listed_rows(graph):
    rowptr, col, val = graph
    x, _ = E.operand(24)
    rows, n_dev = E.row_list()
    assert n_dev < len(rows) and len(set(rows.tolist())) < len(rows)
    dense = E.spmm_mirror(rowptr, col, val, x, 8)
    assert np.array_equal(E.spmm_mirror(rowptr, col, val, x, 8, rows=rows), dense[rows])


def test_exact_case_has_exact_f32_sums():
    rowptr, col, val, x = E.exact_case(24)
    exact, absum, _ = E.spmm_f64(rowptr, col, val, x)
    assert absum.max() < 2.0 ** 24 and np.array_equal(exact * 2.0, np.round(exact * 2.0))   # multiples of 0.5 below 2^24
    for chunk in (None, 8):
        assert np.array_equal(E.spmm_mirror(rowptr, col, val, x, chunk).astype(np.float64), exact)


@pytest.mark.parametrize("K", [0, 1, 2, 3, 4])
def test_read_out_adds_in_the_order_of_the_rule(graph, K):
    """final = c * (E0 + X_1 + ... + X_{K-1} + acc_K): the stored layers rounded, the last one not, left to right."""
    rowptr, col, val = graph
    n = E.N_COLS                                  # a square adjacency: the first 257 rows
    rp = rowptr[: n + 1]
    rng = np.random.default_rng(3)
    e0 = rng.standard_normal((n, 8)).astype(F)
    final, xs, sums = E.propagate_mirror(rp, col, val, e0, K)
    assert len(xs) == (K if K >= 1 else 0) and len(sums) == K + 1
    if K == 0:
        assert np.array_equal(final, e0)
        return
    assert np.array_equal(xs[0], E.rn(e0))
    want = e0.copy()
    for k in range(1, K):
        acc = E.spmm_mirror(rp, col, val, xs[k - 1])
        assert np.array_equal(xs[k], E.rn(acc))                     # stored rounded
        want = (want + xs[k]).astype(F)
        assert np.array_equal(sums[k], want)
    last = E.spmm_mirror(rp, col, val, xs[K - 1])
    want = (want + last).astype(F)                                   # the last layer joins unrounded
    assert np.array_equal(final, (F(1.0 / (K + 1)) * want).astype(F))
    if K >= 2:
        assert not np.array_equal(last, E.rn(last))


def _cpu_trainer(d=16, K=2, **kw):
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    g = t.Generator().manual_seed(0)
    ei = t.stack([t.randint(0, 30, (200,), generator=g), t.randint(0, 20, (200,), generator=g)])
    inter = Interactions(ei, 30, 20)
    return LightGCNTrainer(LightGCN(30, 20, d, K), inter.adjacency("bipartite"), inter, lr=1e-3, Lambda=1e-4, batch_size=32, **kw)


def test_trainer_refusals_name_what_they_refuse():
    with pytest.raises(ValueError, match="layer_dtype must be one of"):
        _cpu_trainer(layer_dtype="fp16")
    with pytest.raises(ValueError, match="multiple of 8"):
        _cpu_trainer(d=20, layer_dtype="bf16")
    with pytest.raises(ValueError, match="stop at d = 256"):
        _cpu_trainer(d=264, layer_dtype="bf16")
    with pytest.raises(ValueError, match="cl_weight"):
        _cpu_trainer(layer_dtype="bf16", sparse_batch=False, cl_weight=0.1)
    # a valid request gets as far as the device check, like the default
    for kw in (dict(layer_dtype="bf16"), dict()):
        with pytest.raises(RuntimeError, match="needs the model on the GPU"):
            _cpu_trainer(**kw)


def test_propagate_mean_and_the_sharded_trainer_refuse():
    from laplace_amd import ops
    from laplace_amd.dist import ShardedLightGCNTrainer
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN, propagate_mean
    e0 = t.zeros(4, 12)
    with pytest.raises(ValueError, match="layer_dtype must be one of"):
        propagate_mean(None, e0, 2, layer_dtype="half")
    with pytest.raises(ValueError, match="multiple of 8"):
        propagate_mean(None, e0, 2, layer_dtype="bf16")
    with pytest.raises(ValueError, match="stop at d = 256"):
        ops.check_bf16_width(512)
    ei = t.stack([t.arange(6) % 3, t.arange(6) % 2])
    with pytest.raises(ValueError, match="layer_dtype"):
        ShardedLightGCNTrainer(LightGCN(3, 2, 8, 1), Interactions(ei, 3, 2), lr=1e-3, Lambda=0.0, batch_size=4, layer_dtype="bf16")


def test_pipeline_and_forward_carry_the_keyword():
    import inspect
    from laplace_amd import run_pipeline_lightgcn as P
    from laplace_amd.model.lightgcn import propagate_mean
    from laplace_amd.trainer import LightGCNTrainer
    for fn in (P.train, propagate_mean, LightGCNTrainer.__init__, LightGCNTrainer.forward):
        assert inspect.signature(fn).parameters["layer_dtype"].default == "f32", fn
    assert "layer_dtype=layer_dtype" in inspect.getsource(P.train)


def test_binding_declares_the_three_entries():
    from laplace_amd import _lib
    L = _lib.lib()
    for name in ("mi_rows_f32_to_bf16", "mi_spmm_csr_bf16", "mi_gather_rows_bf16_f32"):
        assert name in _lib.exported_symbols() and hasattr(L, name)
    # argument checks come before any device work: reachable without a GPU
    assert L.mi_rows_f32_to_bf16(4, 12, None, 12, None, 16, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_spmm_csr_bf16(4, 264, 1, None, None, None, 264, None, 0, None, 0, None, 0, 1.0, None, None, None, 0, 0,
                              None, 0, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_spmm_csr_bf16(4, 20, 1, None, None, None, 24, None, 0, None, 0, None, 0, 1.0, None, None, None, 0, 0,
                              None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_gather_rows_bf16_f32(4, None, 12, None, None, 16, None, 12, 0, None) == _lib.MI_ERR_BAD_ARG
