"""CPU: the table of tests/ranker_step_cases.py against what it was written to cover — both outcomes of every launch kind, every
axis of the executor's branch space — against the executor's own validation pass (mi_ranker_step_check on made-up addresses: a host
walk, nothing enqueued), and the pairing rules restated there against hand-written inputs at every boundary.  A case edited out of
its branch, or a case the executor would decline in silence, fails here before anything runs on a GPU
(tests/test_gpu_ranker_pairs.py runs the same table there).  Also the numpy mirror of the executor's dropout against hand-made
draws."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from laplace_amd import _lib  # noqa: E402
import ranker_dropout_mirror as DM  # noqa: E402
import ranker_step_cases as RC  # noqa: E402
from oracle.philox import philox4x32  # noqa: E402

CSRC = os.path.join(ROOT, "laplace-gnn-recommendation_amd", "csrc")
L = _lib.lib()     # loads without a device: everything called here is a host walk


class Fake:
    """Bump allocator of made-up, 256-byte aligned device addresses (the validation pass dereferences none)."""

    def __init__(self):
        self.at = 0x7F00_0000_0000

    def __call__(self, nbytes):
        p = self.at
        self.at += (int(nbytes) + 255) // 256 * 256 + 256
        return p


@functools.lru_cache(maxsize=None)
def _shapes(name):
    return [RC.batch_shape(b) for b in RC.make_batches(RC.BY_NAME[name])]


def _expected(aux):
    return {c.name: RC.expected_launches(c, aux) for c in RC.CASES}


# ---- the report's layout ------------------------------------------------------------------------------------------------------------
def test_the_kinds_are_the_headers_and_the_bindings():
    header = open(os.path.join(ROOT, "include", "laplace_hip.h")).read()
    enum = re.findall(r"MI_RANKER_LAUNCH_([A-Z0-9_]+) = (\d+)", header)
    assert [k for k, _ in enum] == list(RC.KINDS) + ["KINDS"] and [int(v) for _, v in enum] == list(range(len(RC.KINDS) + 1))
    assert _lib.RANKER_LAUNCH_KINDS == RC.KINDS
    assert ctypes.sizeof(_lib.RankerLaunches) == L.mi_ranker_sizeof(6) == 8 * len(RC.KINDS)
    rep = _lib.RankerLaunches()
    rep.merged[3], rep.single[10] = 7, 9
    assert L.mi_ranker_step_report_f32(None, None, None, 0, None, ctypes.byref(rep)) == -1     # MI_ERR_BAD_ARG ...
    assert rep.as_dict() == {k: (0, 0) for k in RC.KINDS}                                       # ... and the report zeroed first
    assert L.mi_ranker_step_report_f32(None, None, None, 0, None, None) == -1


def test_xcd_ranges_default_is_off():
    """spmm_planless_pair declines under MI_SPMM_XCD_RANGES: the table's spmm expectations hold for the source's default, 0.
    (That the built library has it off is what the merged SPMM counts of tests/test_gpu_ranker_pairs.py show.)"""
    src = open(os.path.join(CSRC, "spmm.hip")).read()
    assert re.search(r"#ifndef MI_SPMM_XCD_RANGES\s*\n#define MI_SPMM_XCD_RANGES 0\s*\n", src)
    assert len(re.findall(r"#\s*define\s+MI_SPMM_XCD_RANGES\b", src)) == 1


# ---- what the table reaches ---------------------------------------------------------------------------------------------------------
def test_both_outcomes_of_every_kind_are_reached():
    twin, aux = _expected(False), _expected(True)
    for kind in RC.KINDS:
        merged = [n for n, e in twin.items() if e[kind][0] > 0]
        assert merged, f"{kind}: no case takes the one-launch form"
        if kind == "LINEAR1_BWD":      # the one-launch form has no decision behind it (pairs.hpp declines null pointers only)
            assert all(e[kind] == (1, 0) for e in list(twin.values()) + list(aux.values()))
            continue
        if kind in ("PREP_DROPOUT", "DROPOUT", "GATHER_CAT_BWD"):   # no shape sends these to single launches: the auxiliary stream does
            assert all(e[kind][1] == 0 for e in twin.values())
            assert any(e[kind][1] > 0 for e in aux.values()), kind
            continue
        assert any(e[kind][1] > 0 for e in twin.values()), f"{kind}: no case falls back to the single launches"
    for name, e in aux.items():
        for kind in RC.TWIN_GATED:
            assert e[kind][0] == 0, (name, kind)
            assert e[kind][1] == sum(twin[name][kind]), (name, kind)       # the same decisions, all single
        for kind in set(RC.KINDS) - set(RC.TWIN_GATED):
            assert e[kind] == twin[name][kind], (name, kind)


def test_the_table_reaches_every_axis():
    cs = RC.CASES
    forms = {RC.embed_pair_form(c.cust_dims, c.art_dims) for c in cs}
    assert forms == {16, 64, None}
    only_article = [c for c in cs if max(c.cust_dims) <= 64 < max(c.art_dims)]
    assert only_article and max(only_article[0].art_dims) == 96
    assert any(max(c.cust_dims) == 96 and max(c.art_dims) == 96 for c in cs)
    assert any(len(c.cust_dims) == RC.MAX_COLS and set(c.cust_dims) == {12} for c in cs)
    assert any(64 in c.cust_dims + c.art_dims for c in cs)                                       # a column of exactly 64
    first = {c.widths for c in cs}
    assert (20, 28) in first and (32, 36) in first
    merged_classes = {RC.lpr_class(a // 4) for a, b in first if RC.spmm_pair_ok(a, b)}
    assert merged_classes == {8, 16, 32, 64}
    assert any(320 in c.conv[:-1] for c in cs)                                                   # d > 256 in a later layer, both directions
    assert {4, 64, 256, 96, 512} <= {c.C for c in cs}
    assert {len(c.conv) for c in cs} == {1, 2, 3} and {c.dec_layers for c in cs} == {1, 2, 3}
    assert any(len(c.conv) == 3 and c.p > 0 for c in cs)                                         # the paired later-layer dropout
    assert any(c.dec_layers == 3 and c.p > 0 for c in cs)                                        # decoder dropout site 65
    assert any(len(c.conv) == 1 and c.p > 0 and c.dec_layers > 1 for c in cs)
    c_outs = {w for c in cs for w in c.conv}
    assert {48, 256} <= c_outs and not RC.wgrad_supported(300, 48, 64, 64) and not RC.wgrad_supported(300, 256, 64, 64)
    l3 = [RC.expected_launches(c, False) for c in cs if len(c.conv) == 3]
    assert any(e["WGRAD"][0] >= 2 for e in l3) and any(e["SPMM_BWD"] == (2, 0) for e in l3)     # per-layer wgrad launches; two merged pairs
    assert {c.aggr for c in cs} == {"add", "mean"} and all(c.isolated for c in cs if c.aggr == "mean")
    assert {c.p for c in cs} == {0.0, 0.3}
    assert sum(c.small_batch for c in cs) == 1 and any(c.odd_grid for c in cs)
    mirrored = [c for c in cs if c.mirror]
    assert all(c.p > 0 for c in mirrored)
    assert {2, 3} <= {len(c.conv) for c in mirrored} and {2, 3} <= {c.dec_layers for c in mirrored}
    assert any((c.C // 4) % 2 == 1 and c.dec_layers > 1 for c in mirrored)
    assert sum(max(c.conv) > 256 for c in cs) >= 2                                               # beyond the widths the float64 bounds were set at
    assert len({c.name for c in cs}) == len(cs) <= 14
    assert sorted(RC.MEASURED) == sorted(c.name for c in cs)                                     # every case has its measured distances on record


# ---- every case is one the executor takes -------------------------------------------------------------------------------------------
def _descriptors(case, shape):
    """The case as mi_ranker_model / mi_ranker_batch on made-up addresses (the validation pass dereferences none)."""
    f = Fake()
    d, b = _lib.RankerModel(), _lib.RankerBatch()
    n_c, n_a, nnz, n_label = shape["n_c"], shape["n_a"], shape["nnz"], shape["n_label"]
    d.n_enc_layers, d.n_dec_layers, d.aggr, d.batch_normalize = len(case.conv), case.dec_layers, int(case.aggr == "mean"), 1
    d.p_dropout, d.max_norm = case.p, 1.0
    for ti, dims in enumerate((case.cust_dims, case.art_dims)):
        d.n_cols[ti] = len(dims)
        for c, w in enumerate(dims):
            d.tables[ti][c], d.table_rows[ti][c], d.dims[ti][c] = f(4 * w * RC.CARDS[c]), RC.CARDS[c], w
    params = []

    def par(n):
        p = (f(4 * n), f(4 * n), f(4 * n), f(4 * n), n)
        params.append(p)
        return p
    for l, ((w_c, w_a), c_out) in enumerate(zip(RC.layer_inputs(case), case.conv)):
        for r, (c_src, c_dst) in enumerate(((w_c, w_a), (w_a, w_c))):
            cv = d.conv[l][r]
            cv.c_src, cv.c_dst, cv.c_out = c_src, c_dst, c_out
            wl, bl, wr = par(c_out * c_src), par(c_out), par(c_out * c_dst)
            cv.w_l, cv.gw_l, cv.b_l, cv.gb_l, cv.w_r, cv.gw_r = wl[0], wl[1], bl[0], bl[1], wr[0], wr[1]
    for ti in range(2):
        nm = d.norm[ti]
        g, be = par(case.C), par(case.C)
        nm.gamma, nm.g_gamma, nm.beta, nm.g_beta = g[0], g[1], be[0], be[1]
        nm.running_mean, nm.running_var, nm.num_batches_tracked = f(4 * case.C), f(4 * case.C), f(8)
        nm.momentum, nm.eps = 0.1, 1e-5
    sizes = [2 * case.C] + [case.dec_hidden] * (case.dec_layers - 1) + [1]
    for j in range(case.dec_layers):
        ln = d.dec[j]
        w, bb = par(sizes[j] * sizes[j + 1]), par(sizes[j + 1])
        ln.w, ln.gw, ln.b, ln.gb = w[0], w[1], bb[0], bb[1]
        ln.in_, ln.out = sizes[j], sizes[j + 1]
    d.n_params, d.apply_adam = len(params), 1
    for i, (p, g, m, v, n) in enumerate(params):
        q = d.params[i]
        q.p, q.g, q.m, q.v, q.n = p, g, m, v, n
    d.lr, d.beta1, d.beta2, d.eps, d.step = 0.01, 0.9, 0.999, 1e-8, 1
    n_ones = max(n_c, n_a, n_label)
    d.ones4, d.n_ones = f(16 * n_ones), n_ones
    b.n_nodes[0], b.n_nodes[1] = n_c, n_a
    b.x[0], b.x[1] = f(8 * n_c * len(case.cust_dims)), f(8 * n_a * len(case.art_dims))
    b.by_customer_ptr, b.by_customer_col = f(4 * (n_c + 1)), f(4 * max(nnz, 1))
    b.by_article_ptr, b.by_article_col = f(4 * (n_a + 1)), f(4 * max(nnz, 1))
    b.nnz, b.n_label = nnz, n_label
    b.label_row, b.label_col, b.label_f32 = f(8 * n_label), f(8 * n_label), f(4 * n_label)
    b.seed, b.step, b.loss = 12345, 7, f(4)
    return d, b, f


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_every_case_is_admitted_by_the_executors_validation_pass(case):
    assert RC.admission_failures(case) == []
    assert _lib.MI_RANKER_MAX_LAYERS == RC.MAX_LAYERS and _lib.MI_RANKER_MAX_COLS == RC.MAX_COLS
    for shape in _shapes(case.name):
        d, b, f = _descriptors(case, shape)
        assert d.n_params <= _lib.MI_RANKER_MAX_PARAMS
        need = int(L.mi_ranker_step_workspace_bytes(ctypes.byref(d), ctypes.byref(b)))
        assert need > 0
        assert L.mi_ranker_step_check(ctypes.byref(d), ctypes.byref(b), f(need), need) == 0
        for aux in (False, True):      # the row counts of the real batches leave wgrad's decision where the table put it
            assert RC.expected_launches(case, aux, (shape["n_c"], shape["n_a"])) == RC.expected_launches(case, aux)


def test_the_restated_admission_conditions_are_the_executors():
    """admission_failures against mi_ranker_step_check on cases just outside: a width that is no multiple of 4, a layer
    input beyond 512, C beyond 512, five layers."""
    from dataclasses import replace
    base, shape = RC.BY_NAME["spmm_8_vs_16_drop"], _shapes("spmm_8_vs_16_drop")[0]
    for bad in (replace(base, cust_dims=(16, 8, 4, 2)), replace(base, conv=(516, 64)), replace(base, conv=(64, 516)),
                replace(base, conv=(64, 62)), replace(base, conv=(8, 8, 8, 8, 8)), replace(base, dec_layers=5)):
        assert RC.admission_failures(bad)
        if len(bad.conv) <= RC.MAX_LAYERS and bad.dec_layers <= RC.MAX_LAYERS:
            d, b, f = _descriptors(bad, shape)
            need = int(L.mi_ranker_step_workspace_bytes(ctypes.byref(d), ctypes.byref(b)))
            assert L.mi_ranker_step_check(ctypes.byref(d), ctypes.byref(b), f(max(need, 256)), max(need, 256)) != 0, bad


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_the_batches_are_what_the_case_needs(case):
    shapes = _shapes(case.name)
    assert len(shapes) == 3
    form = RC.embed_pair_form(case.cust_dims, case.art_dims)
    for s in shapes:
        assert s["n_c"] > 1 and s["n_a"] > 1 and s["nnz"] > 0 and s["n_label"] > 0          # BatchNorm needs two rows
        if not case.small_batch:
            assert s["n_c"] >= 54 and s["n_a"] > 200                                           # _hetero_setup's batches
        if case.isolated:      # mean over an empty row, on both sides: read off the degrees the CSRs are built from
            assert int(s["deg_c"][-1]) == 0 and int(s["deg_a"][-1]) == 0
        if case.small_batch:   # split = 1: the customer side of every twin launch with a split is ONE workgroup
            assert form is not None and RC.embed_grid(s["n_c"], len(case.cust_dims), form) == 1
            assert RC.embed_grid(s["n_a"], len(case.art_dims), form) > 1
            for (w_c, w_a) in RC.layer_inputs(case)[:-1]:
                assert RC.dropout_grid(s["n_c"], w_c) == 1
        if case.odd_grid:
            for n, dims in ((s["n_c"], case.cust_dims), (s["n_a"], case.art_dims)):
                assert (n * len(dims) * 16) % RC.K_BLOCK != 0 and (n * sum(dims) // 4) % RC.K_BLOCK != 0
            if case.p > 0:
                for (w_c, w_a) in RC.layer_inputs(case)[:-1]:
                    assert (s["n_c"] * w_c // 4) % RC.K_BLOCK != 0 and (s["n_a"] * w_a // 4) % RC.K_BLOCK != 0
    assert any(c.isolated for c in RC.CASES)


# ---- the rules at their boundaries ---------------------------------------------------------------------------------------------------
def _case(cust, art, conv=(64,), **kw):
    return RC.Case("hand", tuple(cust), tuple(art), conv=tuple(conv), dec_layers=kw.pop("dec_layers", 2), dec_hidden=16, **kw)


def test_embedding_rule_at_64_and_65():
    assert RC.embed_pair_form((64, 4), (64,)) == 16
    assert RC.embed_pair_form((65, 3), (64,)) is None and RC.embed_pair_form((64,), (4, 65)) is None
    assert RC.embed_pair_form((65,), (4, 65)) == 64
    assert RC.expected_launches(_case((64, 4), (64,)), False)["EMBED"] == (1, 0)
    assert RC.expected_launches(_case((65, 3), (64,)), False)["EMBED"] == (0, 1)
    assert RC.expected_launches(_case((65, 3), (68,)), False)["EMBED"] == (1, 0)
    assert RC.expected_launches(_case((65, 3), (68,)), True)["EMBED"] == (0, 1)


@pytest.mark.parametrize("edge,cls", [(8, 8), (16, 16), (32, 32), (64, 64)])
def test_spmm_rule_at_every_class_boundary(edge, cls):
    """d / 4 of `edge` is the last of its class, edge + 1 the first of the next (or of none: d > 256)."""
    assert RC.lpr_class(edge) == cls and RC.lpr_class(edge + 1) == (2 * cls if cls < 64 else 0)
    lo, hi = 4 * edge, 4 * (edge + 1)
    assert RC.spmm_pair_ok(lo, lo) and not RC.spmm_pair_ok(lo, hi) and RC.spmm_pair_ok(hi, hi) == (cls < 64)
    for widths, first in (((lo, lo), (1, 0)), ((lo, hi), (0, 1)), ((hi, hi), (1, 0) if cls < 64 else (0, 1))):
        e = RC.expected_launches(_case((widths[0],), (widths[1],), conv=(32, 32)), False)
        assert e["SPMM_FWD"] == (first[0] + 1, first[1])                 # layer 1: 32 / 32, merged
        assert e["SPMM_BWD"] == (1, 0)
    e = RC.expected_launches(_case((16,), (16,), conv=(hi, 32, 32)), False)     # the boundary inside: layer 1 forward and backward
    assert e["SPMM_BWD"] == ((2, 0) if cls < 64 else (1, 1)) and e["SPMM_FWD"] == ((3, 0) if cls < 64 else (2, 1))


def test_batchnorm_rule_at_its_boundaries():
    assert [RC.bn_pair_ok(c) for c in (2, 4, 8, 12, 96, 128, 256, 512)] == [False, True, True, False, False, True, True, False]
    for c, want in ((256, (1, 0)), (512, (0, 1)), (4, (1, 0)), (96, (0, 1))):
        e = RC.expected_launches(_case((16,), (16,), conv=(c,)), False)
        assert e["BN_FWD"] == e["BN_BWD"] == want
        e = RC.expected_launches(_case((16,), (16,), conv=(c,)), True)
        assert e["BN_FWD"] == e["BN_BWD"] == (0, 1)


def test_wgrad_rule_and_the_two_forms_of_its_launch():
    assert RC.wgrad_supported(300, 32, 64, 64) and RC.wgrad_supported(300, 128, 512, 512)
    assert not RC.wgrad_supported(300, 160, 64, 64) and not RC.wgrad_supported(300, 48, 64, 64) and not RC.wgrad_supported(300, 64, 516, 64)
    ex = lambda conv: RC.expected_launches(_case((16,), (16,), conv=conv), False)["WGRAD"]   # noqa: E731
    assert ex((64,)) == (1, 0) and ex((48,)) == (0, 1)
    assert ex((64, 64)) == (1, 0) and ex((48, 64)) == (1, 1) and ex((48, 256)) == (0, 2)       # L <= 2: one launch for all
    assert ex((64, 64, 64)) == (3, 0) and ex((64, 320, 64)) == (2, 1)                          # L > 2: one per layer
    assert RC.expected_launches(_case((16,), (16,), conv=(64, 64, 64)), True)["WGRAD"] == (3, 0)   # not a matter of twin()


def test_dropout_kinds_follow_p_and_depth():
    for L_, LD, p, prep, later, gcd in ((1, 1, 0.3, (0, 0), (0, 0), (0, 1)), (1, 2, 0.3, (0, 0), (0, 0), (1, 0)),
                                        (2, 2, 0.3, (1, 0), (0, 0), (1, 0)), (3, 3, 0.3, (1, 0), (1, 0), (1, 0)),
                                        (4, 2, 0.3, (1, 0), (2, 0), (1, 0)), (3, 3, 0.0, (0, 0), (0, 0), (0, 1))):
        c = _case((16,), (16,), conv=(32,) * L_, dec_layers=LD, p=p)
        e, a = RC.expected_launches(c, False), RC.expected_launches(c, True)
        assert (e["PREP_DROPOUT"], e["DROPOUT"], e["GATHER_CAT_DROPOUT"]) == (prep, later, gcd)
        assert (a["PREP_DROPOUT"], a["DROPOUT"], a["GATHER_CAT_DROPOUT"]) == (prep[::-1], later[::-1], gcd)
        assert e["LINEAR1_BWD"] == a["LINEAR1_BWD"] == (1, 0) and e["GATHER_CAT_BWD"] == (1, 0) and a["GATHER_CAT_BWD"] == (0, 1)


# ---- the dropout mirror ---------------------------------------------------------------------------------------------------------------
def test_dropout_mirror_threshold_scale_and_element_order():
    assert DM.threshold(0.3) == 1288490240          # float32(0.3) = 0.300000011920928955 times 2^32, exact in float32
    assert DM.threshold(0.5) == 1 << 31 and DM.threshold(0.0) == 0
    assert DM.threshold(0.99999999) == 4294967040   # float32 rounds p to 1: the clamp below 2^32
    assert DM.scale(0.3) == np.float32(1.0) / np.float32(0.7) and DM.scale(0.5) == 2.0
    seed, step, site, p = (0x1234 << 32) | 0x9ABCDEF0, 7, 65, 0.3
    keep = DM.keep_mask(4 * 1000, p, seed, step, site)
    for i in (0, 5, 999):                            # element 4 i + j is word j of the draw for float4 index i
        words = philox4x32(i, 0, site, step, seed & 0xFFFFFFFF, seed >> 32)
        assert [bool(int(w) >= DM.threshold(p)) for w in words] == keep[4 * i: 4 * i + 4].tolist()
    assert 0.66 < keep.mean() < 0.74
    assert not np.array_equal(keep, DM.keep_mask(4000, p, seed, step, site + 1))
    assert not np.array_equal(keep, DM.keep_mask(4000, p, seed, step + 1, site))
    assert not np.array_equal(keep, DM.keep_mask(4000, p, seed ^ (1 << 40), step, site))     # the high half of the seed is key word 1
    m = DM.multiplier((10, 8), p, seed, step, site)
    assert m.shape == (10, 8) and set(np.unique(m).tolist()) == {0.0, float(DM.scale(p))}
    assert np.array_equal(m.reshape(-1) != 0, keep[:80])
    assert DM.encoder_site(2, 1) == 5 and DM.decoder_site(1) == 65


def test_oracle_twin_runs_with_given_masks():
    """RankerRef.set_dropout_masks: the dropouts multiply by the given multipliers, site by site; None restores F.dropout."""
    import torch as t
    from oracle import ranker_ref as RR
    t.manual_seed(0)
    dims = [{"customer__buys__article": (8, 12, 16), "article__rev_buys__customer": (12, 8, 16)},
            {"customer__buys__article": (16, 16, 4), "article__rev_buys__customer": (16, 16, 4)}]
    ref = RR.RankerRef(dims, [(8, 8), (8, 8), (8, 1)], None, "add", "sum", True, 0.5, 4).double()
    ref.train()
    x = {"customer": t.randn(5, 8, dtype=t.float64), "article": t.randn(7, 12, dtype=t.float64)}
    ei = {("customer", "buys", "article"): t.tensor([[0, 1, 2, 3, 4, 0], [0, 1, 2, 3, 4, 6]]),
          ("article", "rev_buys", "customer"): t.tensor([[0, 1, 2, 3, 4, 6], [0, 1, 2, 3, 4, 0]])}
    eli = t.tensor([[0, 1, 2, 3], [1, 2, 3, 6]])
    ones = {0: t.ones(5, 8), 1: t.ones(7, 12), 64: t.ones(4, 8), 65: t.ones(4, 8)}
    ref.set_dropout_masks({k: v.double() for k, v in ones.items()})
    a = ref(dict(x), ei, eli)
    ref.encoder.p = ref.decoder.p = None            # no dropout at all: the same as all-ones multipliers
    ref.set_dropout_masks(None)
    assert t.equal(a, ref(dict(x), ei, eli))
    ref.encoder.p = ref.decoder.p = 0.5
    for site in ones:                                # every site is read: zeroing one multiplier changes the output
        masks = {k: v.double().clone() for k, v in ones.items()}
        masks[site][:, ::2] = 0.0
        ref.set_dropout_masks(masks)
        assert not t.equal(a, ref(dict(x), ei, eli)), site
    ref.set_dropout_masks({0: ones[0].double()})     # a missing site is an error, not a silent F.dropout
    with pytest.raises(KeyError):
        ref(dict(x), ei, eli)
