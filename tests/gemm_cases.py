"""The case table of the GEMM path tests: one row per call of mi_gemm_f32 (SINGLE) or mi_gemm_group_f32 (GROUPS), each naming
what the dispatcher of csrc/gemm.hip is meant to do with it — the tile kernel (include/laplace_hip.h, MI_GEMM_KERNEL_*), the
K slicing, and for grouped calls the launch, the share set and the workgroup range of every problem.

Two tests read it.  tests/test_gemm_cases_cpu.py asks mi_gemm_plan / mi_gemm_group_plan (host-only, the code the launch
functions themselves call) from made-up addresses with the case's alignment, checks the declarations against the slicing rule
restated below, and checks that the table keeps covering what it was written to cover.  tests/test_gpu_gemm_paths.py builds the
tensors, asks the plan entries again on the real pointers, and compares every output element bitwise with the reference below.

The references.  An unsplit call is ONE k-ascending fma chain per output element (R.gemm_fma), two pairs are one chain over the
concatenated K, then + bias, + C, relu, each one fp32 operation.  A split call is one chain per K slice; the reduce adds every
8th slab in ascending order per group of the 8, the 8 group sums in group order, then the same epilogue
(gemm_splitk_reduce_kernel, gemm_group_reduce_kernel).  A mask SELECTS (a where mask > 0 else 0): a non-finite a behind a closed
entry stays out of the chain.

The float64 bound.  Every fp32 operation rounds once, relative error <= u = 2^-24.  An output element is reached through at most
n = K_total + splits + 3 of them in sequence (the chains of the slices cover K_total fmas between them, at most `splits` adds
join the slabs, then bias, C — and one to spare), so by the standard running-error bound for sums of products
    |got - exact| <= gamma_n * (|op(A)| |op(B)| + |bias| + |C0|),   gamma_n = n u / (1 - n u),
relu being 1-Lipschitz.  No constant here rests on a measurement."""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

NONE, GENERIC, KK, KR, RK, RR = -1, 0, 1, 2, 3, 4          # _lib.MI_GEMM_KERNEL_*
KERNEL_NAMES = {NONE: "none", GENERIC: "generic", KK: "fast<K,K>", KR: "fast<K,R>", RK: "fast<R,K>", RR: "fast<R,R>"}
TRANS = {KK: (False, True), KR: (False, False), RK: (True, True), RR: (True, False)}   # (trans_a, trans_b) of each fast kernel
U = 2.0 ** -24
TILE, MAX_GROUP = 64, 8


# ---- the slicing rule, restated (csrc/gemm.hip: mi_gemm_splits, mi_gemm_decide, group_layout) ---------------------------------
def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def tiles(m: int, n: int) -> int:
    return ceil_div(m, TILE) * ceil_div(n, TILE)


def rule_splits(m: int, n: int, k: int) -> int:
    """Slices asked for.  Outputs of <= 8 tiles: from k = 512 on, >= 128 of k per slice; 9..127 tiles: from k = 2048 on, >= 256."""
    t = tiles(m, n)
    tiny = t <= 8
    if t >= 128 or k < (512 if tiny else 2048):
        return 1
    s = min(ceil_div(512, t), k // (128 if tiny else 256))
    return s if s >= 2 else 1


def slicing(m: int, n: int, k: int, have_ws: bool = True) -> Tuple[int, int]:
    """(splits, k_per_split) as run: slices are whole 32-wide steps; without a workspace one chain."""
    s = rule_splits(m, n, k) if have_ws else 1
    if s == 1:
        return 1, k
    kps = ceil_div(ceil_div(k, s), 32) * 32
    return ceil_div(k, kps), kps


def group_slicing(m: int, n: int, k: int, two_pairs: bool) -> Tuple[int, int]:
    """A grouped problem's own slicing: the single call's, except that a two-pair problem is never split."""
    return (1, k) if two_pairs else slicing(m, n, k)


def unified(members, k: int) -> Tuple[int, int]:
    """A share set's slicing: the coarsest k_per_split of the members' own."""
    kps = max(p for _, p in members)
    return ceil_div(k, kps), kps


def set_workgroups(splits: int, member_tiles) -> int:
    """Slice-major, eight slices abreast: the last group of eight is padded."""
    return ceil_div(splits, 8) * 8 * sum(member_tiles)


# ---- single calls -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Single:
    name: str
    kernel: int                   # declared: the tile kernel this call runs
    splits: int                   # declared: K slices (1 = one chain)
    m: int
    n: int
    k: int
    trans_a: bool
    trans_b: bool
    a_pad: Optional[int] = None   # leading dimension = the operand's stored width + pad; None: the smallest pad that makes it
    b_pad: Optional[int] = None   # a multiple of 4
    a_off: int = 0                # floats between the (256-byte aligned) buffer and the operand's base
    b_off: int = 0
    c_pad: int = 0                # ldc = n + c_pad: C is a column slice of a wider matrix
    bias: bool = False
    accumulate: bool = False
    relu: bool = False
    values: str = "gauss"         # "gauss": randn; "ints": integers of [-2, 2], every sum exact, zeros everywhere

    @property
    def a_width(self) -> int:
        return self.m if self.trans_a else self.k

    @property
    def b_width(self) -> int:
        return self.k if self.trans_b else self.n

    @property
    def lda(self) -> int:
        return self.a_width + ((-self.a_width) % 4 if self.a_pad is None else self.a_pad)

    @property
    def ldb(self) -> int:
        return self.b_width + ((-self.b_width) % 4 if self.b_pad is None else self.b_pad)

    @property
    def ldc(self) -> int:
        return self.n + self.c_pad


EPI = [(b, a, r) for b in (False, True) for a in (False, True) for r in (False, True)]     # (bias, accumulate, relu)
# M, N from {1, 31, 33, 64, 65, 130} (remainders 1, 3, 1, 0, 1, 2 mod 4: the row-contiguous operand's float4 tail);
# K: one panel, panel + 4, a panel's tail, the ranker's widths
SHAPES = [(1, 130, 4), (31, 33, 36), (33, 31, 64), (64, 65, 68), (65, 64, 76), (130, 1, 84), (33, 130, 132), (130, 31, 36)]
# K that only the generic kernel and <false, false> (no K % 4 condition: the odd pairing of the tail) can take
SMALL_K = [(33, 65, 1), (65, 33, 2), (31, 130, 5), (130, 31, 63), (64, 64, 65), (1, 33, 70)]
# (shape, slices): the boundaries of the two split rules, tails, more than 8 slices
SPLIT_SHAPES = [((33, 20, 511), 1), ((33, 20, 512), 4), ((33, 20, 516), 4), ((64, 64, 2560), 20), ((512, 64, 600), 4),
                ((576, 64, 600), 1), ((576, 64, 2047), 1), ((576, 64, 2048), 8), ((576, 64, 2052), 8)]


def _single_cases():
    rows = []
    short = {KK: "kk", KR: "kr", RK: "rk", RR: "rr", GENERIC: "gen"}

    def add(tag, kernel, splits, shape, trans, **kw):
        m, n, k = shape
        rows.append(Single(f"{tag}_m{m}_n{n}_k{k}", kernel, splits, m, n, k, trans[0], trans[1], **kw))

    def epi(i):
        b, a, r = EPI[i % 8]
        return dict(bias=b, accumulate=a, relu=r)

    # -- unsplit, every fast kernel at every K it can take, every epilogue
    for kern in (KK, KR, RK, RR):
        for i, shape in enumerate(SHAPES):
            add(short[kern], kern, 1, shape, TRANS[kern], c_pad=(0, 3)[i % 2], **epi(i))
    for i, shape in enumerate(SMALL_K):
        add("rr_oddk", RR, 1, shape, TRANS[RR], c_pad=(5, 0)[i % 2], values="ints" if shape[2] <= 5 else "gauss", **epi(i + 3))
    # -- unsplit, generic: K % 4 != 0 with a K-contiguous operand, in each transposition that has one; leading dimensions as
    #    they come (a_pad = b_pad = 0: contiguous) and padded to a multiple of 4 (only K is in the way)
    for i, shape in enumerate(SMALL_K):
        pads = dict(a_pad=0, b_pad=0) if i % 2 == 0 else {}
        add(f"gen_oddk_{short[(KK, KR, RK)[i % 3]]}", GENERIC, 1, shape, TRANS[(KK, KR, RK)[i % 3]], c_pad=(0, 2)[i % 2],
            values="ints" if shape[2] <= 5 else "gauss", **pads, **epi(i))
    # -- unsplit, generic at the K every kernel takes: one operand not float4-addressable
    breakers = (("a_ld1", dict(a_pad=1)), ("b_ld1", dict(b_pad=1)), ("a_off1", dict(a_off=1)), ("b_off1", dict(b_off=1)))
    for i, shape in enumerate(SHAPES):
        kern = (KK, KR, RK, RR)[i % 4]
        tag, kw = breakers[(i + i // 4) % 4]
        add(f"gen_{short[kern]}_{tag}", GENERIC, 1, shape, TRANS[kern], c_pad=(3, 0)[i % 2], **kw, **epi(i + 5))
    # -- layouts that move one call between kernels, at one shape per fast kernel
    for j, kern in enumerate((KK, KR, RK, RR)):
        shape, tr = (65, 33, 68), TRANS[kern]
        wa, wb = (shape[0] if tr[0] else shape[2]), (shape[2] if tr[1] else shape[1])
        fit_a, fit_b = (-wa) % 4, (-wb) % 4
        add(f"{short[kern]}_ld4", kern, 1, shape, tr, a_pad=fit_a + 4, b_pad=fit_b + 4, c_pad=7, **epi(j))
        add(f"{short[kern]}_off16", kern, 1, shape, tr, a_off=4, b_off=8, **epi(j + 1))
        add(f"gen_from_{short[kern]}_a_ld1", GENERIC, 1, shape, tr, a_pad=fit_a + 1, c_pad=1, **epi(j + 2))
        add(f"gen_from_{short[kern]}_b_ld1", GENERIC, 1, shape, tr, b_pad=fit_b + 1, **epi(j + 3))
        add(f"gen_from_{short[kern]}_a_off1", GENERIC, 1, shape, tr, a_off=1, **epi(j + 4))
        add(f"gen_from_{short[kern]}_b_off3", GENERIC, 1, shape, tr, b_off=3, c_pad=4, **epi(j + 6))
    # -- split: bias + accumulate + relu into a column slice, each shape in the weight-gradient layout (<false, false>), in the
    #    generic kernel and, where K % 4 == 0, in one of the other three fast kernels in turn
    full = dict(bias=True, accumulate=True, relu=True)
    turn = 0
    for shape, s in SPLIT_SHAPES:
        k = shape[2]
        add("split_rr", RR, s, shape, TRANS[RR], c_pad=4, **full)
        if k % 4:
            add("split_gen_kk", GENERIC, s, shape, TRANS[KK], a_pad=0, b_pad=0, c_pad=1, **full)
            add("split_gen_rk", GENERIC, s, shape, TRANS[RK], c_pad=2, **full)
        else:
            kern = (KK, KR, RK)[turn % 3] if s > 1 else KR
            turn += s > 1
            add(f"split_{short[kern]}", kern, s, shape, TRANS[kern], c_pad=8, **full)
            add(f"split_gen_{short[kern]}_b_off1", GENERIC, s, shape, TRANS[kern], b_off=1, c_pad=3, **full)
    return rows


SINGLE = _single_cases()
SINGLE_BY_NAME = {c.name: c for c in SINGLE}
assert len(SINGLE_BY_NAME) == len(SINGLE)


def expected_kernel(c) -> int:
    """The dispatch rule restated: both operands float4-addressable (16-byte aligned base, leading dimension % 4 == 0) and
    K % 4 == 0 unless both are row-contiguous."""
    a_k, b_k = not c.trans_a, c.trans_b
    ok = c.lda % 4 == 0 and c.ldb % 4 == 0 and c.a_off % 4 == 0 and c.b_off % 4 == 0 and ((not a_k and not b_k) or c.k % 4 == 0)
    if not ok:
        return GENERIC
    return KK if a_k and b_k else KR if a_k else RK if b_k else RR


def single_addresses(c: Single, a_base: int, b_base: int):
    """(A, lda, B, ldb) given the (256-byte aligned) addresses of the two buffers."""
    return a_base + 4 * c.a_off, c.lda, b_base + 4 * c.b_off, c.ldb


# ---- grouped calls ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Prob:
    """One problem of a grouped call.  `a` / `mask` NAME buffers of the call: problems that name the same ones share them (a
    share set needs the same A pointer, K, strides and mask)."""
    m: int
    n: int
    k: int
    trans_a: bool
    trans_b: bool
    a: str
    mask: Optional[str] = None
    k2: int = 0                   # second pair (own A2 / B2), same m, n and trans flags
    bias: bool = False
    accumulate: bool = False
    relu: bool = False
    c_pad: int = 0
    pad: int = 0                  # added to every operand's (multiple-of-4) leading dimension
    # declared
    splits: int = 1               # as run; 0 for an empty problem
    kps: Optional[int] = None     # k_per_split as run (None: k)
    share_set: int = -1           # index within the launch
    first_wg: int = 0
    n_wg: int = 0

    def ld(self, width: int) -> int:
        return width + (-width) % 4 + self.pad

    @property
    def tiles(self) -> int:
        return tiles(self.m, self.n) if self.m and self.n else 0


@dataclass(frozen=True)
class Group:
    name: str
    probs: Tuple[Prob, ...]
    poison: bool = False          # masks get 0.0, -0.0 and negative entries; A gets inf / NaN behind closed entries


def _wgrad(n, k, a, **kw):        # dW = dY^T X: op(A) = dY^T [128, k]
    return Prob(128, n, k, True, False, a, **kw)


_SET_A = dict(splits=58, kps=224, share_set=0, n_wg=640)       # 2 + 8 tiles, own slicings 100 x 128 and 58 x 224; 58 -> 64 slices
GROUPS = [
    # (a) a share set whose members differ in tile count: ONE slicing, the coarsest; the last group of eight slices partly idle
    Group("set_unified_masked", (_wgrad(64, 12_800, "dy", mask="om", **_SET_A), _wgrad(256, 12_800, "dy", mask="om", **_SET_A))),
    Group("set_unified_epilogue", (_wgrad(64, 12_800, "dy", **_SET_A),
                                   _wgrad(256, 12_800, "dy", bias=True, accumulate=True, relu=True, c_pad=4, **_SET_A))),
    # (b) the same set behind an unshared split problem of 5 workgroups: its start is padded to 8; a second set behind it whose
    #     7 slices leave the eighth lane of the XCD row idle
    Group("set_padded_start_two_sets", (
        Prob(64, 64, 640, True, False, "u", splits=5, kps=128, first_wg=0, n_wg=5),
        _wgrad(64, 12_800, "dy", mask="om", **dict(_SET_A, first_wg=8)),
        _wgrad(256, 12_800, "dy", mask="om", bias=True, relu=True, **dict(_SET_A, first_wg=8)),
        Prob(64, 64, 1_100, True, False, "dz", splits=7, kps=160, share_set=1, first_wg=648, n_wg=24),
        Prob(64, 128, 1_100, True, False, "dz", accumulate=True, splits=7, kps=160, share_set=1, first_wg=648, n_wg=24),
        Prob(40, 24, 64, False, True, "sa", accumulate=True, first_wg=672, n_wg=1))),
    # (c) eleven problems, two launches: splits in both (the workspace pointer carries over), an empty problem in the middle,
    #     two-pair problems with the ranker's widths and with two different K tails
    Group("eleven_problems_two_launches", (
        Prob(64, 64, 640, True, False, "u", splits=5, kps=128, first_wg=0, n_wg=5),
        Prob(40, 24, 64, False, True, "sa", accumulate=True, first_wg=5, n_wg=1),
        Prob(130, 128, 76, False, True, "agg", k2=84, bias=True, relu=True, first_wg=6, n_wg=6),
        Prob(0, 128, 76, False, True, "none", splits=0, kps=0, first_wg=12, n_wg=0),
        Prob(130, 76, 128, False, False, "dy2", mask="om2", first_wg=12, n_wg=6),
        Prob(576, 64, 2_052, False, True, "x", bias=True, accumulate=True, relu=True, c_pad=4, splits=8, kps=288,
             first_wg=18, n_wg=72),
        Prob(65, 33, 70, True, False, "t1", first_wg=90, n_wg=2),
        Prob(33, 65, 36, False, False, "t2", relu=True, first_wg=92, n_wg=2),
        Prob(31, 130, 68, True, True, "t3", bias=True, first_wg=0, n_wg=3),
        Prob(33, 20, 516, True, False, "t4", bias=True, accumulate=True, relu=True, c_pad=12, splits=4, kps=160,
             first_wg=3, n_wg=4),
        Prob(65, 70, 68, False, True, "t5", k2=36, accumulate=True, first_wg=7, n_wg=4))),
    # (d) masks with 0.0, -0.0 and negative entries over a K-contiguous A (the dAgg form) and a row-contiguous A, unsplit and
    #     split; inf / NaN in A behind the closed entries
    Group("masks_select", (
        Prob(65, 76, 128, False, False, "dy", mask="om", first_wg=0, n_wg=4),
        Prob(128, 33, 130, True, False, "dy_t", mask="om_t", relu=True, first_wg=4, n_wg=2),
        Prob(64, 20, 516, True, False, "dy_s", mask="om_s", bias=True, splits=4, kps=160, first_wg=6, n_wg=4),
        Prob(33, 20, 640, False, True, "dy_k", mask="om_k", splits=5, kps=128, first_wg=10, n_wg=5)), poison=True),
    # (e) the four operand layouts at M, N, K with remainders, strided, one of them with two pairs
    Group("four_layouts", (
        Prob(65, 33, 76, False, True, "a0", pad=4, bias=True, first_wg=0, n_wg=2),
        Prob(65, 33, 76, False, False, "a1", pad=4, c_pad=3, relu=True, first_wg=2, n_wg=2),
        Prob(65, 33, 76, True, True, "a2", pad=8, k2=84, first_wg=4, n_wg=2),
        Prob(65, 33, 70, True, False, "a3", pad=4, accumulate=True, first_wg=6, n_wg=2))),
]
GROUPS_BY_NAME = {g.name: g for g in GROUPS}
assert len(GROUPS_BY_NAME) == len(GROUPS)


def expected_group_plan(g: Group):
    """The layout pass restated: per problem (launch, splits, k_per_split, share set, first workgroup, workgroups)."""
    out = []
    for base in range(0, len(g.probs), MAX_GROUP):
        ps = g.probs[base:base + MAX_GROUP]
        own = [(0, 0) if not p.tiles else group_slicing(p.m, p.n, p.k, p.k2 > 0) for p in ps]
        key = lambda p: (p.a, p.mask, p.k, p.trans_a, p.pad)
        runs, i = [], 0
        while i < len(ps):                                   # runs of split single-pair problems over one A
            j = i + 1
            while j < len(ps) and own[i][0] > 1 and own[j][0] > 1 and key(ps[i]) == key(ps[j]):
                j += 1
            runs.append((i, j))
            i = j
        at, n_sets = 0, 0
        for i, j in runs:
            if j - i >= 2:
                s, kps = unified(own[i:j], ps[i].k)
                at = ceil_div(at, 8) * 8
                n = set_workgroups(s, [p.tiles for p in ps[i:j]])
                out += [(base // MAX_GROUP, s, kps, n_sets, at, n)] * (j - i)
                at, n_sets = at + n, n_sets + 1
            else:
                s, kps = own[i]
                out.append((base // MAX_GROUP, s, kps, -1, at, ps[i].tiles * s))
                at += ps[i].tiles * s
    return out


def prob_operands(i: int, p: Prob):
    """Buffer names and leading dimensions of problem i of a call (no data)."""
    wa, wb = (p.m if p.trans_a else p.k), (p.k if p.trans_b else p.n)
    rec = dict(a=p.a, mask=p.mask, b=f"b{i}", c=f"c{i}", bias=f"bias{i}" if p.bias else None, lda=p.ld(wa), ldb=p.ld(wb),
               a2=None, b2=None, lda2=0, ldb2=0)
    if p.k2:
        rec.update(a2=f"a2_{i}", b2=f"b2_{i}", lda2=p.ld(p.m if p.trans_a else p.k2), ldb2=p.ld(p.k2 if p.trans_b else p.n))
    return rec


def fill_problems(arr, g: Group, addr):
    """Fills the mi_gemm_problem array `arr` (ctypes, len(g.probs) entries); addr(name) = the address of that buffer."""
    for i, p in enumerate(g.probs):
        r, q = prob_operands(i, p), arr[i]
        q.trans_a, q.trans_b, q.m, q.n, q.k = int(p.trans_a), int(p.trans_b), p.m, p.n, p.k
        q.A, q.lda, q.B, q.ldb = addr(r["a"]), r["lda"], addr(r["b"]), r["ldb"]
        q.k2, q.A2, q.lda2, q.B2, q.ldb2 = p.k2, (addr(r["a2"]) if p.k2 else None), r["lda2"], (addr(r["b2"]) if p.k2 else None), r["ldb2"]
        q.a_mask = addr(p.mask) if p.mask else None
        q.bias = addr(r["bias"]) if p.bias else None
        q.C, q.ldc = addr(r["c"]), p.n + p.c_pad
        q.accumulate, q.act = int(p.accumulate), int(p.relu)
    return arr


def declared_group_plan(g: Group):
    return [(i // MAX_GROUP, p.splits, p.k if p.kps is None else p.kps, p.share_set, p.first_wg, p.n_wg) for i, p in enumerate(g.probs)]


# ---- values and references ----------------------------------------------------------------------------------------------------
def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


def _draw(kind, shape, g):
    import torch as t
    if kind == "ints":
        return t.randint(-2, 3, shape, generator=g).float()
    return t.randn(shape, generator=g)


def _stored(values, ld, off):
    """`values` [rows, width] inside a NaN-filled flat buffer at leading dimension ld, `off` floats in: (buffer, view)."""
    import torch as t
    rows, width = values.shape
    buf = t.full((off + max(rows, 1) * ld + 4,), float("nan"))
    view = buf.as_strided((rows, width), (ld, 1), off)
    view.copy_(values)
    return buf, view


def chain(a_op, b_op):
    """One k-ascending fma chain per element of op(A) [m, k] @ op(B) [k, n]."""
    import torch as t
    from oracle import lightgcn_ref as R
    if a_op.shape[1] == 0:
        return t.zeros(a_op.shape[0], b_op.shape[1])
    return R.gemm_fma(a_op.contiguous(), b_op.contiguous(), trans_a=False, trans_b=False)


def reduce_slabs(slabs, plain_order=False):
    """Every 8th slab in ascending order per group, the 8 group sums in group order (plain_order: a WRONG emulation)."""
    import torch as t
    if plain_order:
        acc = t.zeros_like(slabs[0])
        for s in slabs:
            acc = acc + s
        return acc
    groups = []
    for grp in range(8):
        acc = t.zeros_like(slabs[0])
        for z in range(grp, len(slabs), 8):
            acc = acc + slabs[z]
        groups.append(acc)
    total = groups[0]
    for q in range(1, 8):
        total = total + groups[q]
    return total


def pre_epilogue(a_op, b_op, splits, kps, *, a2_op=None, b2_op=None, plain_order=False):
    """The accumulated product before bias / C / relu: one chain (two pairs: over the concatenated K), or the reduced slabs."""
    import torch as t
    if a2_op is not None:
        assert splits == 1
        return chain(t.cat([a_op, a2_op], 1), t.cat([b_op, b2_op], 0))
    if splits == 1:
        return chain(a_op, b_op)
    k = a_op.shape[1]
    assert ceil_div(k, kps) == splits
    return reduce_slabs([chain(a_op[:, k0:k0 + kps], b_op[k0:k0 + kps]) for k0 in range(0, k, kps)], plain_order)


def epilogue(acc, bias, c0, relu, *, relu_first=False):
    """+ bias, + C, relu: one fp32 operation each, in this order (relu_first: a WRONG emulation, relu before + C)."""
    import torch as t
    v = acc if bias is None else acc + bias
    if relu_first and relu:
        v = t.relu(v)
    if c0 is not None:
        v = v + c0
    return t.relu(v) if relu else v


def split_reference(a_op, b_op, splits, kps, bias=None, c0=None, relu=False):
    """The split-K association of gemm_splitk_reduce_kernel, built from R.gemm_fma."""
    return epilogue(pre_epilogue(a_op, b_op, splits, kps), bias, c0, relu)


def bound(a_op, b_op, bias, c0, k_total, splits):
    """gamma_n * (|op(A)| |op(B)| + |bias| + |C0|), n = K_total + splits + 3, in float64."""
    n = k_total + splits + 3
    gamma = n * U / (1.0 - n * U)
    mag = a_op.double().abs() @ b_op.double().abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    if c0 is not None:
        mag = mag + c0.double().abs()
    return gamma * mag


def exact(a_op, b_op, bias, c0, relu):
    import torch as t
    v = a_op.double() @ b_op.double()
    if bias is not None:
        v = v + bias.double()
    if c0 is not None:
        v = v + c0.double()
    return t.relu(v) if relu else v


def _plant_zeros(c0, pre):
    """Every 7th element of C0 cancels what it is added to exactly: acc + bias + C = 0 there, of either sign nearby."""
    flat, p = c0.view(-1), pre.reshape(-1)
    flat[::7] = -p[::7]


def make_single(c: Single):
    """The case's data on the CPU: the operand buffers in the case's layout (NaN outside the operands), bias, C0 [m, ldc] (NaN
    where accumulate is off), and `want` [m, n], `exact` / `bound` (float64) for the declared slicing."""
    import torch as t
    g = t.Generator().manual_seed(seed_of(c.name))
    a_st = _draw(c.values, (c.k, c.m) if c.trans_a else (c.m, c.k), g)
    b_st = _draw(c.values, (c.n, c.k) if c.trans_b else (c.k, c.n), g)
    a_buf, _ = _stored(a_st, c.lda, c.a_off)
    b_buf, _ = _stored(b_st, c.ldb, c.b_off)
    a_op, b_op = (a_st.t() if c.trans_a else a_st), (b_st.t() if c.trans_b else b_st)
    bias = _draw(c.values, (c.n,), g) if c.bias else None
    splits, kps = c.splits, slicing(c.m, c.n, c.k)[1]
    pre = pre_epilogue(a_op, b_op, splits, kps)
    c0 = None
    if c.accumulate:
        c0 = _draw(c.values, (c.m, c.n), g)
        _plant_zeros(c0, pre if bias is None else pre + bias)
    c_full = t.full((c.m, c.ldc), float("nan"))
    if c0 is not None:
        c_full[:, :c.n] = c0
    return dict(a_buf=a_buf, b_buf=b_buf, bias=bias, c_full=c_full, c0=c0, a_op=a_op, b_op=b_op, pre=pre, kps=kps,
                want=epilogue(pre, bias, c0, c.relu), single_chain=epilogue(chain(a_op, b_op), bias, c0, c.relu),
                exact=exact(a_op, b_op, bias, c0, c.relu), bound=bound(a_op, b_op, bias, c0, c.k, splits))


def _poison(a_st, mask, g):
    """Mask entries exactly 0.0, -0.0 and negative (all closed); inf / NaN in A behind closed entries only."""
    import torch as t
    flat_m, flat_a = mask.view(-1), a_st.view(-1)
    flat_m[0::5] = 0.0
    flat_m[1::5] = -0.0
    flat_m[2::5] = -flat_m[2::5].abs() - 0.5
    closed = (flat_m <= 0).nonzero().view(-1)
    flat_a[closed[0::3]] = float("inf")
    flat_a[closed[1::3]] = float("nan")
    flat_a[closed[2::3]] = -float("inf")


def make_group(gr: Group):
    """The call's data on the CPU.  `buffers`: name -> flat buffer (shared A and mask buffers once); `probs`: per problem the
    buffer names, leading dimensions, bias, C0 in its [m, ldc] frame, the reference operands and want / exact / bound."""
    import torch as t
    g = t.Generator().manual_seed(seed_of(gr.name))
    buffers, stored, out = {}, {}, []
    for i, p in enumerate(gr.probs):
        a_shape = (p.k, p.m) if p.trans_a else (p.m, p.k)
        lda = p.ld(a_shape[1])
        if p.a not in stored:
            a_st = t.randn(a_shape, generator=g)
            stored[p.a] = a_st
            if p.mask is not None:
                mk = t.randn(a_shape, generator=g)
                if gr.poison:
                    _poison(a_st, mk, g)
                stored[p.mask] = mk
                buffers[p.mask] = _stored(mk, lda, 0)[0]
            buffers[p.a] = _stored(a_st, lda, 0)[0]
        a_st = stored[p.a]
        assert tuple(a_st.shape) == a_shape and (p.mask is None or p.mask in stored)
        b_shape = (p.n, p.k) if p.trans_b else (p.k, p.n)
        b_st = t.randn(b_shape, generator=g)
        ldb = p.ld(b_shape[1])
        buffers[f"b{i}"] = _stored(b_st, ldb, 0)[0]
        a_sel = a_st if p.mask is None else t.where(stored[p.mask] > 0, a_st, t.zeros(()))
        a_ge = a_st if p.mask is None else t.where(stored[p.mask] >= 0, a_st, t.zeros(()))        # a WRONG emulation's operand
        op_a = lambda x: x.t() if p.trans_a else x
        a_op, a_op_ge, b_op = op_a(a_sel), op_a(a_ge), (b_st.t() if p.trans_b else b_st)
        rec = prob_operands(i, p)
        assert (rec["lda"], rec["ldb"]) == (lda, ldb)
        a2_op = b2_op = None
        if p.k2:
            a2_st = t.randn((p.k2, p.m) if p.trans_a else (p.m, p.k2), generator=g)
            b2_st = t.randn((p.n, p.k2) if p.trans_b else (p.k2, p.n), generator=g)
            buffers[rec["a2"]] = _stored(a2_st, rec["lda2"], 0)[0]
            buffers[rec["b2"]] = _stored(b2_st, rec["ldb2"], 0)[0]
            a2_op, b2_op = op_a(a2_st), (b2_st.t() if p.trans_b else b2_st)
        bias = t.randn(p.n, generator=g) if p.bias else None
        splits, kps = max(p.splits, 1), (p.k if p.kps is None else p.kps)
        pre = pre_epilogue(a_op, b_op, splits, kps, a2_op=a2_op, b2_op=b2_op) if p.tiles else t.zeros(p.m, p.n)
        c0 = None
        if p.accumulate:
            c0 = t.randn(p.m, p.n, generator=g)
            _plant_zeros(c0, pre if bias is None else pre + bias)
        c_full = t.full((p.m, p.n + p.c_pad), float("nan"))
        if c0 is not None:
            c_full[:, :p.n] = c0
        a_all, b_all = (a_op, b_op) if a2_op is None else (t.cat([a_op, a2_op], 1), t.cat([b_op, b2_op], 0))
        rec.update(bias_t=bias, c_full=c_full, c0=c0, a_op=a_op, b_op=b_op, a2_op=a2_op, b2_op=b2_op, a_op_ge=a_op_ge, pre=pre,
                   want=epilogue(pre, bias, c0, p.relu), exact=exact(a_all, b_all, bias, c0, p.relu),
                   bound=bound(a_all, b_all, bias, c0, p.k + p.k2, splits))
        out.append(rec)
    return dict(buffers=buffers, probs=out)
