"""CPU: which of the five top-K code paths (csrc/topk.hip) every case of tests/topk_cases.py takes, asked of mi_topk_path —
the function the dispatcher of mi_topk_excl_ex_f32 itself calls, host-only — and whether the table still covers what it was
written to cover.  LAPLACE_TOPK_PREFILTER=0 throughout: the prefilter's question to the device (its LDS attribute) is then never
asked, no HIP call is made, and a P case must answer D.  The addresses are made up; mi_topk_path only tests them for alignment.
The conditions below are conditions on the table, not measurements: a case edited out of a path, or a dispatch rule changed
under the table, fails here before anything runs on a GPU (tests/test_gpu_topk_paths.py runs the same table there)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asan_driver import BAD_ARG, L, _lib  # noqa: E402
import topk_cases as T  # noqa: E402

USER_BASE, ITEM_BASE = 0x7F00_0000_0000, 0x7F40_0000_0000    # 256-byte aligned, as the caching allocator's blocks are


@pytest.fixture(autouse=True)
def _prefilter_off(monkeypatch):
    monkeypatch.setenv("LAPLACE_TOPK_PREFILTER", "0")


def _path(c):
    up, ldu, ip, ldi = T.layout_of(c, USER_BASE, ITEM_BASE)
    return int(L.mi_topk_path(c.n_items, c.d, c.k, up, ldu, ip, ldi))


def test_the_constants_of_the_table_are_the_bindings():
    assert (T.M, T.M1, T.G, T.D, T.P) == (_lib.MI_TOPK_PATH_MATERIALISED, _lib.MI_TOPK_PATH_ONE_PASS, _lib.MI_TOPK_PATH_FUSED,
                                          _lib.MI_TOPK_PATH_FUSED_DMA, _lib.MI_TOPK_PATH_PREFILTER)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_every_case_takes_its_declared_path(case):
    assert case.layout in T.LAYOUTS and case.excl in T.EXCLS and case.values in T.VALUES and case.uid in T.UIDS
    got = _path(case)
    assert got == T.expected_path(case, prefilter=False), (case.name, T.PATH_NAMES.get(got, got), T.PATH_NAMES[case.path])


def test_the_rule_itself_at_its_edges():
    """The decision table of include/laplace_hip.h, cell by cell, without the case table in between."""
    a, b = USER_BASE, ITEM_BASE
    path = lambda n, d, k, up=a, ldu=None, ip=b, ldi=None: int(L.mi_topk_path(n, d, k, up, ldu or d, ip, ldi or d))
    assert path(32_767, 64, 12) == T.M and path(32_768, 64, 12) == T.D and path(0, 64, 12) == T.M
    assert path(32_768, 132, 12) == T.M1 and path(32_768, 128, 12) == T.D and path(32_768, 124, 12) == T.G
    assert path(32_768, 30, 12) == T.M1 and path(32_768, 32, 12) == T.G and path(32_768, 4, 12) == T.G
    assert path(40_000, 32, 12, ldu=33) == T.M1 and path(40_000, 32, 12, ldi=33) == T.M1          # either leading dimension
    assert path(40_000, 32, 12, ldu=36, ldi=40) == T.G
    for off in (4, 8, 12):                                                                        # either base
        assert path(40_000, 32, 12, up=a + off) == T.M1 and path(40_000, 32, 12, ip=b + off) == T.M1
    assert path(40_000, 32, 12, up=a + 16, ip=b + 48) == T.G
    assert path(1_000, 32, 12, ip=b + 4) == T.M and path(1_000, 33, 12) == T.M
    assert path(40_000, 64, 256) == T.D and path(40_000, 64, 257) == T.D and path(40_000, 64, 1024) == T.D
    # the negative codes of the main entry
    bad = BAD_ARG
    assert path(-1, 64, 12) == bad and path(100, 0, 12) == bad and path(100, 64, 0) == bad
    assert path(100, 64, 12, up=None) == bad and path(100, 64, 12, ip=None) == bad
    assert path(100, 64, 12, ldu=63) == bad and path(100, 64, 12, ldi=63) == bad
    assert path(100, 64, 1025) == _lib.MI_ERR_UNSUPPORTED
    assert path(2 ** 31 - 1, 64, 12) == -2                                                        # MI_ERR_TOO_LARGE


def test_the_prefilter_switch_is_read_per_call(monkeypatch):
    """Off (the fixture): D without a question to the device.  Any other value: the question is asked, which needs the HIP
    runtime — so only the OFF side and the k > 256 side (never P, whatever the switch says) are pinned here."""
    assert int(L.mi_topk_path(40_000, 128, 12, USER_BASE, 128, ITEM_BASE, 128)) == T.D
    monkeypatch.setenv("LAPLACE_TOPK_PREFILTER", "1")
    assert int(L.mi_topk_path(40_000, 128, 257, USER_BASE, 128, ITEM_BASE, 128)) == T.D
    assert int(L.mi_topk_path(40_000, 32, 12, USER_BASE, 32, ITEM_BASE, 32)) == T.G
    assert int(L.mi_topk_path(40_000, 128, 12, USER_BASE + 4, 128, ITEM_BASE, 128)) == T.M1


# ---- coverage of the table: what each path was promised ---------------------------------------------------------------------
def _of(path):
    return [c for c in T.CASES if c.path == path]


def _has(cases, **want):
    """Is there a case among `cases` with these field values (a set = any of its members, a callable = a predicate)?"""
    def ok(c):
        for f, v in want.items():
            x = getattr(c, f)
            if callable(v):
                if not v(x):
                    return False
            elif isinstance(v, (set, frozenset, tuple)):
                if x not in v:
                    return False
            elif x != v:
                return False
        return True
    return any(ok(c) for c in cases)


def test_every_path_has_its_share_of_cases():
    for path, least in ((T.M, 6), (T.M1, 6), (T.G, 6), (T.D, 6), (T.P, 4)):
        assert len(_of(path)) >= least, T.PATH_NAMES[path]


def test_widths():
    for path, widths in ((T.G, (4, 12, 16, 32, 100, 124)), (T.M1, (132, 200, 256, 512, 33, 50)),
                         (T.M, (1, 3, 50, 100, 200, 512)), (T.D, (64, 128)), (T.P, (64, 128))):
        for d in widths:
            assert _has(_of(path), d=d), (T.PATH_NAMES[path], d)


def test_layouts():
    assert all(_has(T.CASES, layout=l) for l in T.LAYOUTS)
    for path in (T.G, T.D, T.P):                       # ld = d + 4 stays fused
        assert _has(_of(path), layout="ld+4"), T.PATH_NAMES[path]
    for path in (T.M1, T.M):                           # ld = d + 1 and an offset base leave the fused paths
        assert _has(_of(path), layout="ld+1", d=lambda d: d % 4 == 0 and d <= 128), T.PATH_NAMES[path]
        assert _has(_of(path), layout=("off_items", "off_users")), T.PATH_NAMES[path]
    for layout in ("off_items", "off_users", "ld+1_items"):   # either base / one table alone, at a width otherwise fused
        assert _has(_of(T.M1), layout=layout, d=lambda d: d % 4 == 0 and d <= 128), layout
    for path in (T.G, T.M1, T.D, T.P, T.M):
        assert _has(_of(path), layout="halves"), T.PATH_NAMES[path]
    for path in (T.G, T.D, T.P, T.M):                  # PinSAGE.recommend: one table, narrow (G, M) and wide
        assert _has(_of(path), layout="same"), T.PATH_NAMES[path]


def test_item_count_edges():
    assert _has(_of(T.M), n_items=32_767)
    for n in (32_768, 32_769, 32_768 + 63):
        assert _has(_of(T.G), n_items=n) and _has(_of(T.M1), n_items=n), n
        assert _has(_of(T.D) + _of(T.P), n_items=n), n
    for path in (T.G, T.M1, T.D):
        assert _has(_of(path), n_items=105_542), T.PATH_NAMES[path]
    for path in (T.G, T.M1, T.D, T.P):
        for m in (4, 32, 64):
            assert _has(_of(path), n_items=lambda n: n % m != 0), (T.PATH_NAMES[path], m)
    assert _has(_of(T.M1), n_items=50_001, n_q=lambda q: q >= 2)     # row 0 of the score block 16-byte aligned, row 1 not


def test_query_count_edges():
    for n_q in (1, 63, 64, 65, 255, 256, 257):
        assert _has(T.CASES, n_q=n_q), n_q
    for n_q in (63, 64, 65):                           # the 64-query panels of G and D
        assert _has(_of(T.G), n_q=n_q) and _has(_of(T.D), n_q=n_q), n_q
    for n_q in (255, 256, 257):                        # the 256-row strips of P
        assert _has(_of(T.P), n_q=n_q), n_q


def test_k_edges():
    for k in (1, 12, 256, 257, 1024):
        assert _has(T.CASES, k=k), k
    for path in (T.G, T.M1, T.M, T.D):
        assert _has(_of(path), k=1024) and _has(_of(path), k=257), T.PATH_NAMES[path]
    for path in (T.G, T.M1, T.M, T.P):
        assert _has(_of(path), k=1), T.PATH_NAMES[path]
    assert _has(_of(T.P), k=256) and _has(_of(T.D), k=257)           # the two sides of the P / D border
    assert all(c.k > T.PREFILTER_MAX_K for c in _of(T.D)) and all(c.k <= T.PREFILTER_MAX_K for c in _of(T.P))
    assert _has(T.CASES, k=lambda k: k > 700, n_items=700)           # more asked for than exclusion leaves: -1 pads
    assert all(c.k <= c.n_items - T.BEST for c in T.CASES if c.excl == "best")


def test_exclusion_forms_value_kinds_and_queries():
    assert all(_has(T.CASES, excl=e) for e in T.EXCLS)
    assert all(_has(T.CASES, values=v) for v in T.VALUES)
    for path in (T.G, T.M1, T.M, T.D, T.P):
        name = T.PATH_NAMES[path]
        for e in ("none", "dup", "all", "leave_k-1", "best"):
            assert _has(_of(path), excl=e), (name, e)
        for v in ("gauss", "neg", "mixed"):
            assert _has(_of(path), values=v), (name, v)
        assert _has(_of(path), uid="perm") and _has(_of(path), uid="repeat"), name
    for path in (T.G, T.M1, T.M, T.D):
        assert _has(_of(path), excl="empty") and _has(_of(path), values="spread"), T.PATH_NAMES[path]
        assert _has(_of(path), want_scores=False) and _has(_of(path), want_scores=True), T.PATH_NAMES[path]
    # exclusions that land in the sampled runs need a sampled threshold: the paths that take one
    for path in (T.G, T.M1, T.D, T.P):
        assert _has(_of(path), excl="best", n_items=lambda n: n >= T.ONE_PASS_MIN), T.PATH_NAMES[path]
    assert _has(_of(T.G), values="mixed", n_q=lambda q: q > 3)       # fallback rows beside ordinary rows of one panel


def test_chunked_calls():
    for path in (T.M1, T.G):
        assert _has([c for c in _of(path) if c.chunk], chunk=lambda ch: ch > 0), T.PATH_NAMES[path]
    for c in T.CASES:
        if c.chunk:
            assert c.n_q > 2 * c.chunk and c.n_q % c.chunk != 0     # at least three chunks, the last one smaller
