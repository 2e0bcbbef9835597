"""CPU: what the GEMM dispatcher (csrc/gemm.hip) does with every case of tests/gemm_cases.py — the tile kernel and the K slicing,
asked of mi_gemm_plan, and for grouped calls the launch, slicing, share set and workgroup range of every problem, asked of
mi_gemm_group_plan: the host functions the launchers themselves call.  The addresses are made up; the plan entries only test
them for alignment and identity.  No HIP call is made.  The declarations of the table are also held against the slicing rule
restated in gemm_cases.py, the table against what it was written to cover, the references against float64 within the derived
bound, and the bitwise check against six wrong emulations it has to refuse.  A case edited out of its branch, or a dispatch rule
changed under the table, fails here before anything runs on a GPU (tests/test_gpu_gemm_paths.py runs the same table there)."""
import ctypes
import functools
import os
import sys

import pytest
import torch as t

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asan_driver import BAD_ARG, L, _lib  # noqa: E402
import gemm_cases as G  # noqa: E402

A_BASE, B_BASE = 0x7F00_0000_0000, 0x7F40_0000_0000          # 256-byte aligned, as the caching allocator's blocks are
TOO_LARGE, UNSUPPORTED = _lib.MI_ERR_TOO_LARGE, _lib.MI_ERR_UNSUPPORTED


def _plan(trans_a, trans_b, m, n, k, a, lda, b, ldb, gathered=0, ws=1 << 40):
    info = _lib.GemmPlanInfo(77, 77, 77)
    rc = int(L.mi_gemm_plan(int(trans_a), int(trans_b), m, n, k, a, lda, b, ldb, gathered, ws, ctypes.byref(info)))
    return rc, info.kernel, info.splits, info.k_per_split


def _case_plan(c, ws=None):
    a, lda, b, ldb = G.single_addresses(c, A_BASE, B_BASE)
    ws = int(L.mi_gemm_workspace_bytes(c.m, c.n, c.k)) if ws is None else ws
    return _plan(c.trans_a, c.trans_b, c.m, c.n, c.k, a, lda, b, ldb, 0, ws)


@functools.lru_cache(maxsize=None)
def _single(name):
    return G.make_single(G.SINGLE_BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _group(name):
    return G.make_group(G.GROUPS_BY_NAME[name])


def _fake_addresses():
    known = {}

    def addr(name):
        if name not in known:
            known[name] = A_BASE + (len(known) << 32)
        return known[name]
    return addr


def _group_plan(g, mutate=None):
    n = len(g.probs)
    arr = G.fill_problems((_lib.GemmProblem * n)(), g, _fake_addresses())
    if mutate:
        mutate(arr)
    out = (_lib.GemmGroupPlanInfo * n)()
    rc = int(L.mi_gemm_group_plan(arr, n, out))
    return rc, [(o.launch, o.splits, o.k_per_split, o.share_set, o.first_wg, o.n_wg) for o in out], arr


def test_the_constants_of_the_table_are_the_bindings():
    assert (G.NONE, G.GENERIC, G.KK, G.KR, G.RK, G.RR) == (
        _lib.MI_GEMM_KERNEL_NONE, _lib.MI_GEMM_KERNEL_GENERIC, _lib.MI_GEMM_KERNEL_FAST_KK, _lib.MI_GEMM_KERNEL_FAST_KR,
        _lib.MI_GEMM_KERNEL_FAST_RK, _lib.MI_GEMM_KERNEL_FAST_RR)
    assert ctypes.sizeof(_lib.GemmPlanInfo) == 16 and ctypes.sizeof(_lib.GemmGroupPlanInfo) == 40
    assert _lib.MI_ABI_VERSION == 14 and L.mi_abi_version() == 14                          # additive: the version stays


# ---- every case takes its declared branch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SINGLE, ids=lambda c: c.name)
def test_every_single_case_runs_its_declared_kernel_and_slicing(case):
    c = case
    assert c.lda >= c.a_width and c.ldb >= c.b_width
    splits, kps = G.slicing(c.m, c.n, c.k)
    assert c.splits == splits, "the declaration against the rule restated"
    assert c.kernel == G.expected_kernel(c), (G.KERNEL_NAMES[c.kernel], G.KERNEL_NAMES[G.expected_kernel(c)])
    rc, kernel, got_s, got_kps = _case_plan(c)
    assert rc == 0 and kernel == c.kernel, (G.KERNEL_NAMES.get(kernel, kernel), G.KERNEL_NAMES[c.kernel])
    assert (got_s, got_kps) == (splits, kps)
    # the short-workspace fallback: none, and one byte less than the slabs need -> one chain, the same kernel
    need = G.rule_splits(c.m, c.n, c.k) * c.m * c.n * 4
    for ws in (0, need - 1):
        assert _case_plan(c, ws=ws) == (0, c.kernel, 1, c.k)
    if splits > 1:
        assert int(L.mi_gemm_workspace_bytes(c.m, c.n, c.k)) >= need and _case_plan(c, ws=need) == (0, c.kernel, splits, kps)
        assert c.k - (splits - 1) * kps > 0 and kps % 32 == 0


@pytest.mark.parametrize("group", G.GROUPS, ids=lambda g: g.name)
def test_every_grouped_case_gets_its_declared_layout(group):
    declared = G.declared_group_plan(group)
    assert declared == G.expected_group_plan(group), "the declaration against the layout pass restated"
    rc, got, arr = _group_plan(group)
    assert rc == 0 and got == declared
    assert L.mi_gemm_group_supported(arr, len(group.probs)) == 1
    # the workspace the launch asks for holds every slab of the slicing it runs (slabs are sized by the members' own slicing)
    need = sum((p.splits * p.m * p.n * 4 + 255) // 256 * 256 for p in group.probs if p.splits > 1)
    assert int(L.mi_gemm_group_workspace_bytes(arr, len(group.probs))) >= need
    # ranges of one launch do not overlap, sets start on a multiple of 8
    for launch in {d[0] for d in declared}:
        spans = sorted({(d[4], d[5], d[3]) for d in declared if d[0] == launch and d[5] > 0})
        for (s0, n0, _), (s1, _, set1) in zip(spans, spans[1:]):
            assert s0 + n0 <= s1 and (set1 < 0 or s1 % 8 == 0) and s1 - (s0 + n0) < 8


# ---- coverage of the table ------------------------------------------------------------------------------------------------------
def _of(kernel, split=None):
    return [c for c in G.SINGLE if c.kernel == kernel and (split is None or (c.splits > 1) == split)]


def test_every_kernel_split_and_unsplit_at_every_k_and_remainder():
    every, odd = (4, 36, 64, 68, 76, 84, 132), (1, 2, 5, 63, 65, 70)
    for kern in (G.GENERIC, G.KK, G.KR, G.RK, G.RR):
        name = G.KERNEL_NAMES[kern]
        un = _of(kern, split=False)
        assert len(_of(kern, split=True)) >= 2 and len(un) >= 10, name
        assert {c.k for c in un} >= set(every), name
        assert {c.m for c in un} >= {1, 31, 33, 64, 65, 130} and {c.n for c in un} >= {1, 31, 33, 64, 65, 130}, name
        assert {(c.bias, c.accumulate, c.relu) for c in un} == set(G.EPI), name
        assert any(c.c_pad > 0 for c in un) and any(c.c_pad == 0 for c in un), name
    for kern in (G.GENERIC, G.RR):
        assert {c.k for c in _of(kern, split=False)} >= set(odd), G.KERNEL_NAMES[kern]
    # the row-contiguous operand's float4 tail: widths with remainder 1, 2, 3 mod 4, on either side
    for kern, side in ((G.RK, "m"), (G.RR, "m"), (G.KR, "n"), (G.RR, "n")):
        assert {getattr(c, side) % 4 for c in _of(kern, split=False)} >= {0, 1, 2, 3}, (G.KERNEL_NAMES[kern], side)
    assert all(c.k % 4 == 0 for kern in (G.KK, G.KR, G.RK) for c in _of(kern))


def test_layouts_that_move_a_call_between_kernels():
    for kern in (G.KK, G.KR, G.RK, G.RR):
        fast, tr = _of(kern), G.TRANS[kern]
        assert any(c.lda > c.a_width + 3 and c.ldb > c.b_width + 3 for c in fast), "ld + 4 stays fast"
        assert any(c.a_off and c.b_off for c in fast), "a base 16 bytes into a buffer stays fast"
        gen = [c for c in _of(G.GENERIC) if (c.trans_a, c.trans_b) == tr and c.k % 4 == 0]
        assert any(c.lda % 4 for c in gen) and any(c.ldb % 4 for c in gen), G.KERNEL_NAMES[kern]
        assert any(c.a_off % 4 for c in gen) and any(c.b_off % 4 for c in gen), G.KERNEL_NAMES[kern]
    assert any(c.trans_a and c.lda % 4 for c in _of(G.GENERIC))                            # row-contiguous A, lda % 4 != 0


def test_split_cases_reach_both_rules_their_borders_and_more_than_eight_slices():
    split = [c for c in G.SINGLE if c.name.startswith("split_")]
    shapes = {(c.m, c.n, c.k): c.splits for c in split}
    assert shapes == dict(G.SPLIT_SHAPES)
    assert all(c.bias and c.accumulate and c.relu and c.c_pad > 0 for c in split)
    for shape in shapes:
        rows = [c for c in split if (c.m, c.n, c.k) == shape]
        assert len({c.kernel for c in rows}) >= 2 and any(c.kernel == G.GENERIC for c in rows), shape
    tiny = [c for c in split if c.splits > 1 and G.tiles(c.m, c.n) <= 8]
    wide = [c for c in split if c.splits > 1 and G.tiles(c.m, c.n) > 8]
    assert tiny and wide and any(c.splits > 8 for c in split)
    assert any(c.k % G.slicing(c.m, c.n, c.k)[1] == 36 for c in tiny) and any(c.k % G.slicing(c.m, c.n, c.k)[1] == 36 for c in wide)
    for kern in (G.GENERIC, G.KK, G.KR, G.RK, G.RR):
        assert any(c.kernel == kern for c in tiny + wide), G.KERNEL_NAMES[kern]


def test_grouped_cases_reach_what_they_were_written_for():
    probs = [(g, i, p) for g in G.GROUPS for i, p in enumerate(g.probs)]
    member = [(g, i, p) for g, i, p in probs if p.share_set >= 0]
    # a set with unified slicing: a member whose own slicing differs from what it runs, and a padded last group of eight slices
    assert any(G.group_slicing(p.m, p.n, p.k, False) != (p.splits, p.kps) for _, _, p in member)
    assert any(p.splits % 8 for _, _, p in member) and any(p.splits > 8 for _, _, p in member)
    assert any(p.mask for _, _, p in member) and any(p.bias and p.accumulate and p.relu for _, _, p in member)
    # a padded set start, two sets in one launch
    assert any(p.first_wg > 0 and p.first_wg % 8 == 0 and
               any(q.share_set < 0 and 0 < q.first_wg + q.n_wg < p.first_wg and q.first_wg + q.n_wg > p.first_wg - 8
                   for q in g.probs[:i]) for g, i, p in member)
    assert any(len({p.share_set for p in g.probs[:8] if p.share_set >= 0}) == 2 for g in G.GROUPS)
    # a second launch with a split problem, a split problem in the first of the same call, an empty problem, pairs
    assert any(len(g.probs) > 8 and any(p.splits > 1 for p in g.probs[:8]) and any(p.splits > 1 for p in g.probs[8:]) and
               any(p.m == 0 for p in g.probs[1:-1]) for g in G.GROUPS)
    assert any(p.k2 and (p.k, p.k2) == (76, 84) for _, _, p in probs)
    assert any(p.k2 and p.k % 64 and p.k2 % 64 and p.k % 64 != p.k2 % 64 for _, _, p in probs)
    # an unshared split problem with the whole epilogue; masks on both A layouts, poisoned; the four layouts
    assert any(p.share_set < 0 and p.splits > 1 and p.bias and p.accumulate and p.relu for _, _, p in probs)
    assert any(g.poison and p.mask and not p.trans_a for g, _, p in probs) and any(g.poison and p.mask and p.trans_a for g, _, p in probs)
    assert any(g.poison and p.mask and p.splits > 1 for g, _, p in probs)
    assert {(p.trans_a, p.trans_b) for _, _, p in probs if p.m % 4 and p.n % 4} == set(G.TRANS.values())


# ---- the references against float64, within the derived bound ---------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SINGLE, ids=lambda c: c.name)
def test_single_reference_is_within_the_derived_bound_of_float64(case):
    d = _single(case.name)
    assert bool(t.isfinite(d["want"]).all())
    assert bool(((d["want"].double() - d["exact"]).abs() <= d["bound"]).all())
    assert bool(((d["single_chain"].double() - d["exact"]).abs() <= d["bound"]).all())
    if case.accumulate:                                              # acc + bias + C exactly 0, and negative, are both there
        pre = d["pre"] if d["bias"] is None else d["pre"] + d["bias"]
        v = pre + d["c0"]
        assert int((v == 0).sum()) >= v.numel() // 7 and bool((v < 0).any())
        assert bool((d["want"].view(-1)[::7] == 0).all())


@pytest.mark.parametrize("group", G.GROUPS, ids=lambda g: g.name)
def test_grouped_references_are_within_the_derived_bound_of_float64(group):
    for p, r in zip(group.probs, _group(group.name)["probs"]):
        assert bool(t.isfinite(r["want"]).all())
        assert bool(((r["want"].double() - r["exact"]).abs() <= r["bound"]).all()), (p.m, p.n, p.k)


# ---- the bitwise check refuses wrong emulations ---------------------------------------------------------------------------------
def test_bias_added_per_slice_is_refused():
    c = G.SINGLE_BY_NAME["split_rr_m33_n20_k516"]
    d = _single(c.name)
    kps = d["kps"]
    slabs = [G.chain(d["a_op"][:, k0:k0 + kps], d["b_op"][k0:k0 + kps]) + d["bias"] for k0 in range(0, c.k, kps)]
    wrong = G.epilogue(G.reduce_slabs(slabs), None, d["c0"], c.relu)
    assert not t.equal(wrong, d["want"])
    slabs = [G.chain(d["a_op"][:, k0:k0 + kps], d["b_op"][k0:k0 + kps]) + d["bias"] / c.splits for k0 in range(0, c.k, kps)]
    assert not t.equal(G.epilogue(G.reduce_slabs(slabs), None, d["c0"], c.relu), d["want"])


@pytest.mark.parametrize("name", ["kk_m64_n65_k68", "split_rr_m64_n64_k2560"])
def test_relu_before_plus_c_is_refused(name):
    c, d = G.SINGLE_BY_NAME[name], _single(name)
    assert c.accumulate and c.relu
    assert not t.equal(G.epilogue(d["pre"], d["bias"], d["c0"], True, relu_first=True), d["want"])


def test_pairs_swapped_are_refused():
    g = G.GROUPS_BY_NAME["eleven_problems_two_launches"]
    hit = 0
    for p, r in zip(g.probs, _group(g.name)["probs"]):
        if p.k2:
            swapped = G.pre_epilogue(r["a2_op"], r["b2_op"], 1, p.k2, a2_op=r["a_op"], b2_op=r["b_op"])
            assert not t.equal(G.epilogue(swapped, r["bias_t"], r["c0"], p.relu), r["want"])
            hit += 1
    assert hit == 2


def test_mask_greater_or_equal_zero_is_refused():
    g = G.GROUPS_BY_NAME["masks_select"]
    for p, r in zip(g.probs, _group(g.name)["probs"]):
        wrong = G.epilogue(G.pre_epilogue(r["a_op_ge"], r["b_op"], max(p.splits, 1), p.kps or p.k), r["bias_t"], r["c0"], p.relu)
        assert not t.equal(wrong, r["want"]) and not bool(t.isfinite(wrong).all())


def test_slabs_summed_in_plain_order_are_refused():
    c = G.SINGLE_BY_NAME["split_rr_m64_n64_k2560"]
    d = _single(c.name)
    assert c.splits == 20
    wrong = G.epilogue(G.pre_epilogue(d["a_op"], d["b_op"], 20, d["kps"], plain_order=True), d["bias"], d["c0"], c.relu)
    assert not t.equal(wrong, d["want"])
    assert not t.equal(d["single_chain"], d["want"])                # nor is a split result the single chain


def test_members_sliced_separately_are_refused():
    g = G.GROUPS_BY_NAME["set_unified_epilogue"]
    p, r = g.probs[0], _group(g.name)["probs"][0]
    own_s, own_kps = G.group_slicing(p.m, p.n, p.k, False)
    assert (own_s, own_kps) == (100, 128) and (p.splits, p.kps) == (58, 224)
    wrong = G.epilogue(G.pre_epilogue(r["a_op"], r["b_op"], own_s, own_kps), r["bias_t"], r["c0"], p.relu)
    assert not t.equal(wrong, r["want"])


# ---- the rule itself, cell by cell ------------------------------------------------------------------------------------------------
def test_the_rule_itself_at_its_edges():
    a, b = A_BASE, B_BASE

    def plan(m, n, k, ta=False, tb=True, pa=a, lda=None, pb=b, ldb=None, gathered=0, ws=1 << 40):
        lda = lda or (m if ta else k)
        ldb = ldb or (k if tb else n)
        rc, kern, s, kps = _plan(ta, tb, m, n, k, pa, lda, pb, ldb, gathered, ws)
        return (kern, s, kps) if rc == 0 else rc
    # the kernel: alignment of either base, either leading dimension, K % 4, the row gather
    assert plan(64, 64, 64) == (G.KK, 1, 64) and plan(64, 64, 64, tb=False) == (G.KR, 1, 64)
    assert plan(64, 64, 64, ta=True) == (G.RK, 1, 64) and plan(64, 64, 64, ta=True, tb=False) == (G.RR, 1, 64)
    for off in (4, 8, 12):
        assert plan(64, 64, 64, pa=a + off)[0] == G.GENERIC and plan(64, 64, 64, pb=b + off)[0] == G.GENERIC
    assert plan(64, 64, 64, pa=a + 16, pb=b + 48)[0] == G.KK
    for ta, tb in G.TRANS.values():
        for d in (1, 2, 3):
            assert plan(64, 64, 64, ta, tb, lda=64 + d)[0] == G.GENERIC and plan(64, 64, 64, ta, tb, ldb=64 + d)[0] == G.GENERIC
        assert plan(64, 64, 64, ta, tb, lda=68, ldb=72)[0] != G.GENERIC
    for k in (1, 2, 3, 5, 6, 7, 63, 65, 66):
        assert plan(64, 64, k)[0] == plan(64, 64, k, tb=False, ldb=64)[0] == plan(64, 64, k, ta=True, lda=64)[0] == G.GENERIC
        assert plan(64, 64, k, ta=True, tb=False, lda=64, ldb=64)[0] == G.RR
    assert plan(64, 64, 64, gathered=1)[0] == G.KK and plan(64, 64, 64, tb=False, gathered=1)[0] == G.KR      # K-contiguous rows: a map is fine
    assert plan(64, 64, 64, ta=True, gathered=1)[0] == G.GENERIC and plan(64, 64, 64, ta=True, tb=False, gathered=1)[0] == G.GENERIC
    # the tiny rule: <= 8 tiles, from k = 512 on, >= 128 per slice, at most ceil(512 / tiles) slices
    assert plan(64, 64, 511)[1:] == (1, 511) and plan(64, 64, 512)[1:] == (4, 128) and plan(64, 64, 639)[1:] == (4, 160)
    assert plan(64, 64, 640)[1:] == (5, 128) and plan(1, 1, 1 << 20)[1:] == (512, 2048)
    assert plan(512, 64, 1 << 20)[1:] == (64, 16384) and plan(64, 512, 600)[1:] == (4, 160) and plan(128, 256, 600)[1:] == (4, 160)
    # the wider rule: 9 .. 127 tiles, from k = 2048 on, >= 256 per slice
    assert plan(576, 64, 600)[1:] == (1, 600) and plan(513, 64, 2047)[1:] == (1, 2047) and plan(513, 64, 2048)[1:] == (8, 256)
    assert plan(576, 64, 1 << 20)[1:] == (57, 18400) and plan(64, 127 * 64, 1 << 20)[1:] == (5, 209728)
    assert plan(64, 127 * 64, 2048)[1:] == (5, 416) and plan(64, 128 * 64, 1 << 20)[1:] == (1, 1 << 20)   # 127 tiles split, 128 do not
    assert plan(64 * 8, 64 * 16, 1 << 20)[1:] == (1, 1 << 20) and plan(127 * 64 + 1, 64, 4096)[1:] == (1, 4096)
    # the workspace: the slabs of the slices ASKED for must fit, else one chain
    assert plan(64, 64, 512, ws=4 * 64 * 64 * 4) == (G.KK, 4, 128) and plan(64, 64, 512, ws=4 * 64 * 64 * 4 - 1) == (G.KK, 1, 512)
    assert plan(64, 64, 512, ws=0) == (G.KK, 1, 512)
    # nothing to do, and the negative codes of mi_gemm_f32
    assert plan(0, 64, 64) == (G.NONE, 0, 0) and plan(64, 0, 64, ldb=64) == (G.NONE, 0, 0) and plan(64, 64, 0, lda=4, ldb=4)[1:] == (1, 0)
    bad = BAD_ARG
    assert plan(-1, 64, 64) == bad and plan(64, -1, 64) == bad and plan(64, 64, -1) == bad
    assert plan(64, 64, 64, pa=None) == bad and plan(64, 64, 64, pb=None) == bad
    assert plan(64, 64, 64, lda=63) == bad and plan(64, 64, 64, ldb=63) == bad
    assert plan(60, 64, 64, ta=True, lda=59) == bad and plan(64, 60, 64, tb=False, ldb=59) == bad
    assert int(L.mi_gemm_plan(0, 1, 64, 64, 64, a, 64, b, 64, 0, 0, None)) == bad
    assert plan(65_535 * 64, 1, 4)[0] == G.KK and plan(65_535 * 64 + 1, 1, 4) == TOO_LARGE
    assert plan(65_535 * 64 + 1, 1, 4, ta=True) == TOO_LARGE


def test_the_grouped_rule_at_its_edges():
    # a two-pair problem is never split, whatever its k
    g = G.Group("x", (G.Prob(64, 64, 4096, True, False, "a", k2=4096),))
    assert _group_plan(g)[1] == [(0, 1, 4096, -1, 0, 1)]
    # a set needs the same A, k, strides and mask: each difference alone dissolves it
    two = lambda **kw: G.Group("x", (G.Prob(64, 64, 1100, True, False, "a"), G.Prob(64, 128, 1100, True, False, **{"a": "a", **kw})))
    assert [d[3] for d in _group_plan(two())[1]] == [0, 0]
    assert [d[3] for d in _group_plan(two(a="other"))[1]] == [-1, -1]
    assert [d[3] for d in _group_plan(two(mask="om"))[1]] == [-1, -1]
    assert [d[3] for d in _group_plan(two(pad=4))[1]] == [-1, -1]
    assert [d[:4] for d in _group_plan(two(k2=64))[1]] == [(0, 7, 160, -1), (0, 1, 1100, -1)]
    # unsplit problems over one A form no set; nor does a single split problem
    g = G.Group("x", (G.Prob(64, 64, 76, True, False, "a"), G.Prob(64, 128, 76, True, False, "a")))
    assert [d[3] for d in _group_plan(g)[1]] == [-1, -1]
    # at most four sets per launch: a fifth run is laid problem after problem
    g = G.Group("x", tuple(G.Prob(64, 64, 640, True, False, f"a{i // 2}") for i in range(8)) +
                (G.Prob(64, 64, 640, True, False, "a3"), G.Prob(64, 64, 640, True, False, "a3")))
    got = _group_plan(g)[1]
    assert [d[3] for d in got] == [0, 0, 1, 1, 2, 2, 3, 3, 0, 0] and [d[0] for d in got] == [0] * 8 + [1] * 2
    assert [d[4] for d in got] == [0, 0, 16, 16, 32, 32, 48, 48, 0, 0] and all(d[5] == 16 for d in got)
    # the negative codes, for the whole call, wherever the problem sits
    group = G.GROUPS_BY_NAME["eleven_problems_two_launches"]
    for i in (0, 5, 9, 10):
        for what in ("A", "B", "lda", "ldb", "k"):
            def mutate(arr, i=i, what=what):
                setattr(arr[i], what, getattr(arr[i], what) + (4 if what in ("A", "B") else 1))
            p = group.probs[i]
            rr = p.trans_a and not p.trans_b
            want = 0 if (what == "k" and rr) else UNSUPPORTED
            rc, _, arr = _group_plan(group, mutate)
            assert rc == want and L.mi_gemm_group_supported(arr, 11) == (1 if want == 0 else 0), (i, what)
    def mask_off(arr):
        arr[4].a_mask += 8
    assert _group_plan(group, mask_off)[0] == UNSUPPORTED
    def bad_act(arr):
        arr[9].act = 2
    assert _group_plan(group, bad_act)[0] == BAD_ARG
    def null_c(arr):
        arr[8].C = None
    assert _group_plan(group, null_c)[0] == UNSUPPORTED
    assert int(L.mi_gemm_group_plan(None, 1, None)) == BAD_ARG and int(L.mi_gemm_group_plan(None, 0, None)) == 0
    assert int(L.mi_gemm_group_plan(None, -1, None)) == BAD_ARG
    arr = G.fill_problems((_lib.GemmProblem * 11)(), group, _fake_addresses())
    assert int(L.mi_gemm_group_plan(arr, 11, None)) == BAD_ARG
    # the launch entry refuses the same calls with the same codes before it lays anything out (no device is touched)
    for mutate, want in ((mask_off, UNSUPPORTED), (bad_act, BAD_ARG), (null_c, UNSUPPORTED)):
        arr = G.fill_problems((_lib.GemmProblem * 11)(), group, _fake_addresses())
        mutate(arr)
        assert int(L.mi_gemm_group_f32(arr, 11, None, 0, None)) == want
