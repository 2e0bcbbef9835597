"""The case table of the top-K path tests: one row per call of ops.topk_excl, each naming the code path of
csrc/topk.hip it is meant to hit (include/laplace_hip.h, mi_topk_path: M, M1, G, D, P).

Two tests read it.  tests/test_topk_paths_cpu.py asks mi_topk_path (host-only) for every case's path from made-up addresses
with the same alignment, and checks that the table keeps covering what it was written to cover.  tests/test_gpu_topk_paths.py
builds the tensors, asks ops.topk_path again on the real pointers and compares ids and scores of every query row with the
oracle's fma chain.  A plain module, no fixtures: a case is data, and `layout_of` / `build` turn it into addresses / tensors.

Non-finite embeddings are outside K10's contract (include/laplace_hip.h) and therefore outside this table."""
from dataclasses import dataclass
from typing import Optional

M, M1, G, D, P = 0, 1, 2, 3, 4     # _lib.MI_TOPK_PATH_*
PATH_NAMES = {M: "M", M1: "M1", G: "G", D: "D", P: "P"}
ONE_PASS_MIN = 32_768              # 8 * kSample of csrc/topk.hip: rows this long leave the materialised multi-pass path
PREFILTER_MAX_K = 256              # kPreMaxK of csrc/topk_prefilter.hpp
BEST = 200                         # exclusion form "best": a row's exclusions are exactly its BEST best items

LAYOUTS = ("contig",       # two contiguous tables
           "ld+4",         # row-strided views, ld = d + 4: float4-addressable, stays fused
           "ld+1",         # ld = d + 1: rows not float4-addressable, leaves the fused paths
           "ld+1_items",   # only the item table has ld = d + 1, the user table is contiguous: the same
           "off_items",    # the item table starts one float into a larger buffer (base not 16-byte aligned)
           "off_users",    # the same for the user table
           "halves",       # fin[:U], fin[U:] of one table: the propagated predictor's form
           "same")         # one tensor passed as both tables: PinSAGE.recommend's form
EXCLS = ("none",           # excl=None
         "empty",          # a CSR whose rows are all empty: excl_idx is null
         "random",         # up to 400 random ids per row, unsorted
         "dup",            # random ids, every one of them listed twice (repeated purchases), unsorted
         "all",            # row 0 excludes every item (comes back all -1), the others random
         "leave_k-1",      # row 0 excludes all but k - 1 items, the others random
         "best")           # every row excludes exactly its BEST best items (by the oracle's ranking): they sit wherever the
                           # sample runs are as well, and must not lift the sampled threshold
VALUES = ("gauss",         # randn * 0.1
          "neg",           # ue = rand + 0.5, ie = -(rand + 0.5): every score negative
          "pos",           # ue = rand + 0.5, ie = rand + 0.5: every score positive
          "spread",        # components +-10^[-15, 15]: keys ordered across exponents, no overflow (d * 1e30 < f32 max)
          "mixed")         # gaussian tables, but every third query user is all zeros (every score +0: one n_items-way tie)
                           # and every third + 1 has one non-zero component against an item column of three values (three
                           # huge tie groups): fallback rows beside ordinary rows of the same 64-query panel
UIDS = ("perm",            # distinct users in random order
        "repeat")          # drawn with replacement; uid[1] = uid[0]


@dataclass(frozen=True)
class Case:
    name: str
    path: int
    n_items: int
    n_q: int
    d: int
    k: int
    layout: str = "contig"
    excl: str = "random"
    values: str = "gauss"
    uid: str = "perm"
    want_scores: bool = True
    chunk: Optional[int] = None    # also run cut into chunks of this many queries (2 streams, 1 stream): same bits

    @property
    def n_users(self) -> int:
        return self.n_items if self.layout == "same" else self.n_q + 37


CASES = [
    # ---- G: fused, generic kernel (fused-eligible, d neither 64 nor 128) -------------------------------------------------
    Case("g_d4_one_query", G, 32_768, 1, 4, 1, excl="none"),
    Case("g_d12_pinsage_form", G, 40_000, 65, 12, 12, layout="same", uid="repeat"),
    Case("g_d16_strided_dup_neg", G, 32_769, 63, 16, 256, layout="ld+4", excl="dup", values="neg"),
    Case("g_d32_bench_catalogue_best", G, 105_542, 64, 32, 12, layout="halves", excl="best"),
    Case("g_d100_partial_panel_chunked", G, 32_768 + 63, 257, 100, 100, chunk=100),
    Case("g_d124_spread_k257_all", G, 40_002, 255, 124, 257, layout="ld+4", excl="all", values="spread"),
    Case("g_d32_mixed_fallback_rows", G, 33_333, 70, 32, 50, values="mixed"),
    Case("g_d16_k1024_pos_ids_only", G, 36_001, 41, 16, 1024, excl="empty", values="pos", want_scores=False),
    Case("g_d100_leave_k-1", G, 32_800, 5, 100, 12, excl="leave_k-1", uid="repeat"),
    Case("g_d32_256_queries", G, 32_768, 256, 32, 1, excl="none", values="neg"),
    # ---- M1: materialised, one collect pass (n_items >= 32 768, not fused-eligible) --------------------------------------
    Case("m1_d132_threshold", M1, 32_768, 64, 132, 12),
    Case("m1_d200_odd_rows_best", M1, 50_001, 41, 200, 256, excl="best"),          # row 0 16-byte aligned, row 1 not
    Case("m1_d256_chunked_dup", M1, 40_000, 257, 256, 1, excl="dup", chunk=100),
    Case("m1_d512_bench_catalogue", M1, 105_542, 41, 512, 12, layout="halves", excl="none"),
    Case("m1_d33_slow_gemm_neg", M1, 33_333, 63, 33, 100, values="neg", uid="repeat"),
    Case("m1_d50_spread_k257", M1, 32_769, 65, 50, 257, values="spread"),
    Case("m1_d64_ld_plus_1", M1, 40_000, 41, 64, 12, layout="ld+1"),
    Case("m1_d128_items_offset", M1, 50_001, 2, 128, 256, layout="off_items", excl="empty"),
    Case("m1_d32_users_offset", M1, 32_768 + 63, 255, 32, 12, layout="off_users", values="pos"),
    Case("m1_d132_mixed_all", M1, 34_002, 70, 132, 50, excl="all", values="mixed"),
    Case("m1_d50_k1024_leave_k-1_ids_only", M1, 36_001, 5, 50, 1024, excl="leave_k-1", want_scores=False),
    Case("m1_d16_ld_plus_1", M1, 33_000, 63, 16, 12, layout="ld+1", excl="none"),
    Case("m1_d32_items_ld_plus_1", M1, 32_768, 65, 32, 12, layout="ld+1_items"),
    # ---- M: materialised, multi-pass (n_items < 32 768) ------------------------------------------------------------------
    Case("m_d1", M, 1_000, 65, 1, 12),
    Case("m_d3_just_below_threshold", M, 32_767, 64, 3, 256, values="pos"),
    Case("m_d50_k1024", M, 5_000, 256, 50, 1024, excl="dup"),
    Case("m_d100_k_beyond_what_is_left", M, 700, 63, 100, 1024),                   # <= 700 items left: the tail is -1 pads
    Case("m_d200_items_offset", M, 3_001, 41, 200, 12, layout="off_items", excl="all"),
    Case("m_d512", M, 2_000, 41, 512, 1, excl="none", values="neg"),
    Case("m_d64_ld_plus_1", M, 20_000, 41, 64, 12, layout="ld+1", excl="best"),
    Case("m_d16_pinsage_form", M, 3_000, 257, 16, 12, layout="same", uid="repeat", want_scores=False),
    Case("m_d100_halves_mixed", M, 4_097, 70, 100, 50, layout="halves", excl="leave_k-1", values="mixed"),
    Case("m_d128_spread", M, 32_767, 1, 128, 257, excl="empty", values="spread"),
    # ---- D: fused, LDS-DMA kernel (d 64 / 128, k > 256 here; every P case below also runs D with the prefilter off) -------
    Case("d_d64_k257", D, 32_768, 65, 64, 257),
    Case("d_d128_k257_strided", D, 32_769, 64, 128, 257, layout="ld+4", excl="dup"),
    Case("d_d128_k1024_bench_catalogue", D, 105_542, 41, 128, 1024, layout="halves", excl="best"),
    Case("d_d64_k1024_neg_ids_only", D, 40_002, 63, 64, 1024, values="neg", excl="none", want_scores=False),
    Case("d_d128_mixed_k300", D, 32_768 + 63, 70, 128, 300, values="mixed", excl="all"),
    Case("d_d64_same_tensor_k257", D, 33_333, 257, 64, 257, layout="same", uid="repeat", excl="leave_k-1"),
    Case("d_d64_spread_k512", D, 50_001, 1, 64, 512, values="spread", excl="empty"),
    # ---- P: bf16x3 prefilter (d 64 / 128, k <= 256) -----------------------------------------------------------------------
    Case("p_d64_k256_strided", P, 32_768, 63, 64, 256, layout="ld+4"),
    Case("p_d128_k1_halves_257_queries", P, 32_768 + 63, 257, 128, 1, layout="halves", excl="dup"),
    Case("p_d128_k12_best_256_queries", P, 40_002, 256, 128, 12, excl="best"),
    Case("p_d64_pinsage_form", P, 33_333, 255, 64, 12, layout="same", uid="repeat", excl="all"),
    Case("p_d128_neg_leave_k-1", P, 50_001, 65, 128, 256, values="neg", excl="leave_k-1"),
    Case("p_d64_mixed", P, 32_769, 70, 64, 100, values="mixed", excl="none"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def layout_of(c: Case, user_base: int, item_base: int):
    """(user_ptr, ldu, item_ptr, ldi) of the case's two tables, given the (256-byte aligned) base addresses of the buffers
    `build` allocates for them.  "halves" and "same" keep both tables in the user buffer."""
    ld = {"ld+4": c.d + 4, "ld+1": c.d + 1, "ld+1_items": c.d + 1}.get(c.layout, c.d)
    up, ip = user_base, item_base
    if c.layout == "off_items":
        ip += 4
    elif c.layout == "off_users":
        up += 4
    elif c.layout == "halves":
        ip = user_base + 4 * c.n_users * c.d
    elif c.layout == "same":
        ip = user_base
    return up, (c.d if c.layout == "ld+1_items" else ld), ip, ld


def expected_path(c: Case, prefilter: bool) -> int:
    """The declared path; with the prefilter switched off a P case runs D."""
    return D if (c.path == P and not prefilter) else c.path


def _values(c: Case, g, n_rows_u: int, n_rows_i: int):
    import torch as t
    d = c.d
    if c.values in ("gauss", "mixed"):
        ue, ie = t.randn(n_rows_u, d, generator=g) * 0.1, t.randn(n_rows_i, d, generator=g) * 0.1
    elif c.values == "neg":
        ue, ie = t.rand(n_rows_u, d, generator=g) + 0.5, -(t.rand(n_rows_i, d, generator=g) + 0.5)
    elif c.values == "pos":
        ue, ie = t.rand(n_rows_u, d, generator=g) + 0.5, t.rand(n_rows_i, d, generator=g) + 0.5
    elif c.values == "spread":
        def spread(n):
            mag = 10.0 ** (t.rand(n, d, generator=g, dtype=t.float64) * 30.0 - 15.0)
            sign = t.randint(0, 2, (n, d), generator=g).double() * 2.0 - 1.0
            return (mag * sign).float()
        ue, ie = spread(n_rows_u), spread(n_rows_i)
    else:
        raise ValueError(c.values)
    return ue, ie


def build(c: Case, device: str):
    """The case's tensors.  Returns a dict: ue / ie (device views in the case's layout), ue_ref / ie_ref (contiguous CPU copies
    of the same values, for the oracle), uid (CPU int64), excl (CPU list of int64 id tensors per query, or None),
    rowptr / col (CPU int32 CSR of the same lists in the order they are given to the device, or None) and `need_scores`:
    True when `excl` still waits for the oracle's scores (form "best": call finish_excl)."""
    import torch as t
    g = t.Generator().manual_seed(hash_name(c.name))
    U, I, d = c.n_users, c.n_items, c.d
    if c.layout == "same":
        assert c.values in ("gauss", "pos", "spread")   # a table against itself: the sign of a score is not ours to choose
        _, ie_ref = _values(c, g, 1, I)
        ue_ref = ie_ref
    else:
        ue_ref, ie_ref = _values(c, g, U, I)
    uid = t.randperm(U, generator=g)[:c.n_q] if c.uid == "perm" else t.randint(0, U, (c.n_q,), generator=g)
    if c.uid == "repeat" and c.n_q > 1:
        uid[1] = uid[0]
    if c.values == "mixed":
        assert c.layout != "same"
        ie_ref[:, 0] = t.randint(-1, 2, (I,), generator=g).float() * 0.5
        users = uid.clone()
        ue_ref[users[0::3]] = 0.0
        one = users[1::3]
        keep = ue_ref[one, 0].clone()
        ue_ref[one] = 0.0
        ue_ref[one, 0] = keep
    # ---- the device tensors in the case's layout
    ld = {"ld+4": d + 4, "ld+1": d + 1, "ld+1_items": d + 1}.get(c.layout, d)

    def strided(x):
        buf = t.full((x.shape[0], ld), float("nan"), device=device)   # the gaps are never to be read
        buf[:, :d] = x.to(device)
        return buf[:, :d]

    def offset(x):
        buf = t.full((x.numel() + 1,), float("nan"), device=device)
        buf[1:] = x.to(device).reshape(-1)
        return buf[1:].view(x.shape)

    if c.layout in ("ld+4", "ld+1"):
        ue, ie = strided(ue_ref), strided(ie_ref)
    elif c.layout == "ld+1_items":
        ue, ie = ue_ref.to(device), strided(ie_ref)
    elif c.layout == "off_items":
        ue, ie = ue_ref.to(device), offset(ie_ref)
    elif c.layout == "off_users":
        ue, ie = offset(ue_ref), ie_ref.to(device)
    elif c.layout == "halves":
        fin = t.cat([ue_ref, ie_ref]).to(device)
        ue, ie = fin[:U], fin[U:]
    elif c.layout == "same":
        ue = ie = ie_ref.to(device)
    else:
        ue, ie = ue_ref.to(device), ie_ref.to(device)
    out = dict(ue=ue, ie=ie, ue_ref=ue_ref, ie_ref=ie_ref, uid=uid, excl=None, rowptr=None, col=None, need_scores=False)
    # ---- exclusions
    if c.excl == "none":
        return out
    if c.excl == "best":
        out["need_scores"] = True
        return out
    lists = []
    for q in range(c.n_q):
        if c.excl == "empty":
            lists.append(t.empty(0, dtype=t.int64))
            continue
        n = int(t.randint(0, min(I, 400), (1,), generator=g))
        e = t.randperm(I, generator=g)[:n]
        if c.excl == "dup":
            e = t.cat([e, e])[t.randperm(2 * n, generator=g)]
        lists.append(e)
    if c.excl == "all":
        lists[0] = t.randperm(I, generator=g)
    elif c.excl == "leave_k-1":
        lists[0] = t.randperm(I, generator=g)[: I - (c.k - 1)]
    _set_excl(out, lists)
    return out


def finish_excl(c: Case, b: dict, scores) -> None:
    """Exclusion form "best": `scores` are the oracle's [n_q, n_items]; every row excludes exactly its BEST best items."""
    import torch as t
    assert c.excl == "best" and b["need_scores"]
    g = t.Generator().manual_seed(hash_name(c.name) + 1)
    lists = []
    for q in range(c.n_q):
        top = scores[q].topk(BEST).indices
        lists.append(top[t.randperm(BEST, generator=g)])
    _set_excl(b, lists)
    b["need_scores"] = False


def _set_excl(b: dict, lists) -> None:
    import torch as t
    b["excl"] = lists
    lens = t.tensor([len(e) for e in lists], dtype=t.int64)
    b["rowptr"] = t.cat([t.zeros(1, dtype=t.int64), lens.cumsum(0)]).to(t.int32)
    b["col"] = t.cat(lists).to(t.int32)


def hash_name(name: str) -> int:
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h
