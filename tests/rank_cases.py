"""The case table of the full-rank tests: one row per call of ops.rank_of_items, each naming the code path of csrc/rank.hip it
is meant to hit (include/laplace_hip.h, mi_rank_path: F fused, M materialised).

A case carries the fields of a tests/topk_cases.py case (name, n_items, n_q, d, k, layout, excl, values, uid, n_users), so
topk_cases.build / finish_excl / layout_of make its tensors and addresses; `path` is the RANK path.  `k` only shapes the
exclusion form "leave_k-1" (row 0 keeps k - 1 items) and the width of the top-K lists in the agreement test.  `targets`
draws the case's target items.  tests/test_full_rank_cpu.py asks mi_rank_path for every case's path from made-up addresses and
checks the coverage; tests/test_gpu_full_rank.py runs the table on the device against tests/full_rank_reference.py.
Nothing is larger than 40 002 items x 257 rows.  Non-finite embeddings are outside the contract and outside this table."""
from dataclasses import dataclass

import topk_cases as T

M, F = 0, 1                      # _lib.MI_RANK_PATH_MATERIALISED, _lib.MI_RANK_PATH_FUSED
PATH_NAMES = {M: "M", F: "F"}


@dataclass(frozen=True)
class Case:
    name: str
    path: int
    n_items: int
    n_q: int
    d: int
    k: int = 12
    layout: str = "contig"
    excl: str = "random"
    values: str = "gauss"
    uid: str = "perm"

    @property
    def n_users(self) -> int:
        return self.n_items if self.layout == "same" else self.n_q + 37


CASES = [
    # ---- F: fused (d <= 128, d % 4 == 0, float4-addressable rows, 16-byte aligned bases), any number of items --------------
    Case("f_one_item_d4", F, 1, 63, 4, 1, excl="all"),                       # row 0 excludes the only item
    Case("f_63_items_d12_pinsage_form", F, 63, 65, 12, 12, layout="same", excl="dup", uid="repeat"),
    Case("f_64_items_d64_one_query_strided", F, 64, 1, 64, 12, layout="ld+4", excl="none"),
    Case("f_65_items_d100_halves_mixed", F, 65, 63, 100, 12, layout="halves", values="mixed"),
    Case("f_4097_items_d128_mixed_leave_k-1", F, 4_097, 257, 128, 50, excl="leave_k-1", values="mixed"),
    Case("f_4097_items_d4_pos_none", F, 4_097, 65, 4, 12, excl="none", values="pos", uid="repeat"),
    Case("f_partial_last_tile_d64_best", F, 32_768 + 63, 65, 64, 12, excl="best"),
    Case("f_40002_items_d128_spread_all", F, 40_002, 257, 128, 12, layout="ld+4", excl="all", values="spread"),
    Case("f_40002_items_d64_neg_empty", F, 40_002, 63, 64, 12, excl="empty", values="neg", uid="repeat"),
    Case("f_40002_items_d12_halves_dup", F, 40_002, 1, 12, 12, layout="halves", excl="dup"),
    Case("f_32831_items_d100_same_spread", F, 32_768 + 63, 63, 100, 12, layout="same", values="spread", uid="repeat"),
    Case("f_64_items_d128_mixed_none", F, 64, 257, 128, 12, excl="none", values="mixed"),
    # ---- M: materialised (every other width or layout) ----------------------------------------------------------------------
    Case("m_d1", M, 1_000, 65, 1, 12),
    Case("m_d33_mixed_dup", M, 4_097, 63, 33, 12, excl="dup", values="mixed", uid="repeat"),
    Case("m_d132_all", M, 5_000, 257, 132, 12, excl="all"),
    Case("m_d200_spread_best", M, 3_001, 41, 200, 12, excl="best", values="spread"),
    Case("m_d64_ld_plus_1_none", M, 40_002, 41, 64, 12, layout="ld+1", excl="none"),
    Case("m_d64_items_ld_plus_1_leave_k-1", M, 4_097, 65, 64, 30, layout="ld+1_items", excl="leave_k-1", values="neg"),
    Case("m_d64_items_offset_empty", M, 32_768 + 63, 1, 64, 12, layout="off_items", excl="empty"),
    Case("m_d64_users_offset_pos", M, 65, 63, 64, 12, layout="off_users", values="pos"),
    Case("m_one_item_d33", M, 1, 5, 33, 1, excl="all", uid="repeat"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

layout_of = T.layout_of          # (user_ptr, ldu, item_ptr, ldi) from two 256-byte aligned bases: the same rule
build = T.build
finish_excl = T.finish_excl

KINDS = ("best", "worst", "random", "excluded", "tie_middle", "minus_one", "n_items")


def targets(c: Case, scores, excl):
    """int64 [n_q] target items and the kind of each (a list of KINDS names), drawn from a generator seeded by the case's
    name and mixed within the case.  scores: the reference's [n_q, n_items]; excl: a list of id tensors per row, or None.
      best / worst   the admissible item top-K's order puts first / last
      random         any admissible item
      excluded       an item of the row's exclusion list (rank -1), where the row has one
      tie_middle     ("mixed" cases) an admissible item from the middle of the row's largest group of equal scores
      minus_one, n_items   out of range (rank -1, score 0)
    A kind a row cannot serve (nothing admissible, nothing excluded) falls back to "random", then to "excluded"."""
    import numpy as np
    import torch as t
    rng = np.random.default_rng(T.hash_name(c.name) + 7)
    kinds_here = [k for k in KINDS if k != "tie_middle" or c.values == "mixed"]
    ids = np.arange(c.n_items)
    out, kinds = [], []
    for q in range(c.n_q):
        kind = kinds_here[(q + int(rng.integers(0, 2))) % len(kinds_here)]
        s = scores[q].numpy().astype(np.float64) + 0.0
        mask = np.ones(c.n_items, dtype=bool)
        if excl is not None and len(excl[q]):
            mask[excl[q].numpy()] = False
        adm = ids[mask]
        if kind in ("best", "worst", "random", "tie_middle") and adm.size == 0:
            kind = "excluded"
        if kind == "excluded" and mask.all():
            kind = "random"
        if kind == "minus_one":
            tgt = -1
        elif kind == "n_items":
            tgt = c.n_items
        elif kind == "excluded":
            gone = ids[~mask]
            tgt = int(gone[rng.integers(0, gone.size)])
        elif kind == "random":
            tgt = int(adm[rng.integers(0, adm.size)])
        elif kind == "tie_middle":
            vals, inverse, counts = np.unique(s[adm], return_inverse=True, return_counts=True)
            group = adm[inverse == int(counts.argmax())]            # ascending ids
            tgt = int(group[group.size // 2])
        else:
            order = np.lexsort((adm, -s[adm]))                      # score desc, id asc
            tgt = int(adm[order[0 if kind == "best" else -1]])
        out.append(tgt)
        kinds.append(kind)
    return t.tensor(out, dtype=t.int64), kinds
