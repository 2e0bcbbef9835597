"""The cases of tests/test_gpu_ranker_pairs.py and the pairing rules of the native ranker executor restated in Python.

csrc/ranker_exec.hip issues the customer-side and the article-side twin of a step as ONE launch where the two sides share a
kernel instantiation (csrc/pairs.hpp), else — and always with the auxiliary stream, LAPLACE_RANKER_AUX=1 — as two single
launches.  Both forms give the same bits; mi_ranker_step_report_f32 says which one ran.  `expected_launches(case, aux)` is what
that report must hold, derived from the sources:

  EMBED (sage.hip: embed_concat_pair)   merged with the 16-lane kernel when every column of BOTH sides is <= 64 wide; merged with
                                        the 64-lane kernel when EACH side has a column of its own wider than 64; single when only
                                        one side has one (the single launches would pick different instantiations).
  SPMM_FWD / SPMM_BWD (spmm.hip: spmm_planless_pair, lpr_class)   merged when d / 4 of both sides falls in the same class of
                                        <= 8, <= 16, <= 32, <= 64; single when the classes differ or d > 256.  The pair launcher
                                        also declines under MI_SPMM_XCD_RANGES, whose compile-time default is 0 (spmm.hip:
                                        test_ranker_step_cases_cpu.py reads it there).  Forward: one decision per
                                        layer, d = the two types' input widths.  Backward: layers l > 0 only (layer 0 reads frozen
                                        tables), d = that layer's input width on both sides.
  BN_FWD / BN_BWD (norm.hip: bn_pow2_rows)   merged when C is a power of two in 4..256; else the single launches (generic kernel
                                        for a C that is no power of two, and for C = 512).
  PREP_DROPOUT                          the first layer's two input dropouts ride in the prep launch when p > 0 and L > 1.
  DROPOUT                               a later layer's two input dropouts, 0 < l < L - 1, as one launch.
  GATHER_CAT_DROPOUT                    merged (the gather draws the decoder's first dropout itself) when p > 0 and LD > 1, else
                                        the plain gather; LINEAR1_BWD always the one-launch form.  Neither asks twin(): the same
                                        count with and without the auxiliary stream.
  GATHER_CAT_BWD                        always one launch for both sums.
  WGRAD (wgrad.hip: mi_sage_wgrad_supported)   a layer takes the transposed-product kernel when c_out is a multiple of 32 and
                                        <= 128 (and c_src, c_dst <= 512): merged counts that kernel's LAUNCHES — one for all such
                                        layers when L <= 2, one per layer when L > 2 — single counts the layers that went through
                                        the grouped GEMM.  Not asked of twin() either.
  With aux=True every kind that asks twin() reports merged == 0.

Importable without a GPU: the batches come from the host sampler.  The graph is tests/test_gpu_ranker.py::_hetero_setup's
(400 customers, 120 articles, 3000 edges; 6 seeds, 2 hops of 8 — 54 customers and ~300 articles per batch), except for the one
case that needs a customer side of a single workgroup, which 54 customers cannot give (54 x 16 lanes > 256): it samples 1 seed
with 2 neighbours (3 customers).

The distances to the float64 oracle measured on an MI355X are recorded per case in MEASURED below.
"""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch as t

KINDS = ("EMBED", "PREP_DROPOUT", "DROPOUT", "SPMM_FWD", "BN_FWD", "GATHER_CAT_DROPOUT", "LINEAR1_BWD", "GATHER_CAT_BWD", "BN_BWD",
         "SPMM_BWD", "WGRAD")
TWIN_GATED = ("EMBED", "PREP_DROPOUT", "DROPOUT", "SPMM_FWD", "BN_FWD", "GATHER_CAT_BWD", "BN_BWD", "SPMM_BWD")   # ask twin()
K_BLOCK = 256                 # workgroup size of the embedding, dropout and prep kernels
MAX_LAYERS, MAX_COLS = 4, 16  # MI_RANKER_MAX_LAYERS, MI_RANKER_MAX_COLS
# cardinality of categorical column i (either side): table i has this many rows
CARDS = (300, 2, 84, 4, 5, 2, 7, 19, 100, 132, 30, 50, 3, 11, 64, 9)


@dataclass(frozen=True)
class Case:
    name: str
    cust_dims: Tuple[int, ...]      # embedding width of every customer column
    art_dims: Tuple[int, ...]
    conv: Tuple[int, ...]           # c_out of every encoder layer (the last one is C)
    dec_layers: int                 # LD
    dec_hidden: int
    aggr: str = "add"
    p: float = 0.0
    small_batch: bool = False       # 1 seed, 2 neighbours per hop: a customer side of ONE workgroup
    isolated: bool = False          # append one edgeless node of each type (mean over an empty row)
    mirror: bool = False            # one of the cases test_dropout_masks_are_the_mirrored_ones must run
    odd_grid: bool = False          # neither side's element count is a multiple of 256 (asserted on the batches)

    @property
    def widths(self) -> Tuple[int, int]:
        return sum(self.cust_dims), sum(self.art_dims)

    @property
    def C(self) -> int:
        return self.conv[-1]


CASES: List[Case] = [
    # L = 1, LD = 1, C = 4: no dropout site at all, no backward product, linear1_bwd the only decoder backward; first-layer spmm 20 / 28:
    # class 8, partly filled
    Case("l1_ld1_c4", (8, 4, 4, 4), (16, 8, 4), conv=(4,), dec_layers=1, dec_hidden=8, odd_grid=True),
    # first-layer spmm 32 / 36: classes 8 and 16, the fallback; later layer class 16; prep + dropout merged; fused gather dropout
    Case("spmm_8_vs_16_drop", (16, 8, 4, 4), (16, 8, 8, 4), conv=(64, 64), dec_layers=2, dec_hidden=128, p=0.3, mirror=True),
    # class 16 (48 / 64, a column of exactly 64); mean with an empty row on each side; C = 256: BatchNorm merged, wgrad's c_out = 256
    # goes through the grouped GEMM while layer 0 (c_out = 128) takes the transposed-product kernel
    Case("class16_mean_c256", (32, 16), (64,), conv=(128, 256), dec_layers=2, dec_hidden=64, aggr="mean", isolated=True),
    # class 32 (100 / 128); c_out = 48: wgrad through the grouped GEMM; C = 96: BatchNorm's generic single launches; LD = 3 without dropout
    Case("class32_c48_c96_ld3", (64, 36), (64, 64), conv=(48, 96), dec_layers=3, dec_hidden=32),
    # both sides own a 96-wide column: the 64-lane embedding pair; class 64 (132 / 256); mean + dropout
    Case("wide_cols_both_mean_drop", (96, 36), (96, 96, 64), conv=(64, 64), dec_layers=2, dec_hidden=128, aggr="mean", p=0.3,
         isolated=True),
    # only the article side owns a 96-wide column: embedding fallback; 32 / 128: classes 8 and 32; L = 1 with p > 0: no encoder dropout,
    # but the fused gather dropout
    Case("wide_col_article_only", (16, 16), (96, 32), conv=(32,), dec_layers=2, dec_hidden=16, p=0.3),
    # 16 columns (MI_RANKER_MAX_COLS) of width 12: four idle lanes per sub-group of the 16-lane kernel; class 64 (192 / 136)
    Case("sixteen_cols_w12", (12,) * 16, (60, 64, 8, 4), conv=(64, 64), dec_layers=2, dec_hidden=128),
    # hidden 320: every later layer's forward and backward product has d > 256 (fallback); L = 3: per-layer wgrad launches (c_out = 64
    # only; 320 through the GEMM), the paired later-layer dropout
    Case("hidden320_l3_drop", (8, 4, 4, 4), (16, 8, 4), conv=(320, 320, 64), dec_layers=2, dec_hidden=32, p=0.3, mirror=True),
    # L = 3, LD = 3, C = 20 (C / 4 = 5: the gather's column arithmetic on a width that is no power of two; BatchNorm generic); two merged
    # backward spmm pairs (classes 16 and 8); wgrad per layer for 32 and 64, GEMM for 20; decoder dropout sites 64 and 65
    Case("l3_ld3_c20_drop", (12, 12), (20, 8), conv=(32, 64, 20), dec_layers=3, dec_hidden=24, p=0.3, mirror=True, odd_grid=True),
    # C = 512: BatchNorm single launches at the executor's limit; class 16 (48 / 64)
    Case("c512", (24, 24), (40, 24), conv=(512,), dec_layers=2, dec_hidden=8),
    # L = 2, LD = 2, C = 12 (C / 4 = 3) with dropout
    Case("c12_drop", (8, 8, 4), (16, 16), conv=(16, 12), dec_layers=2, dec_hidden=12, p=0.3, mirror=True),
    # 3 customers: ONE workgroup on the customer side of the embedding pair (3 x 3 sub-groups of 16 lanes), of prep + dropout and of the
    # later layer's dropout pair (split = 1); L = 3
    Case("one_workgroup_l3_drop", (8, 4, 4), (16, 8, 8), conv=(16, 16, 8), dec_layers=2, dec_hidden=8, p=0.3, small_batch=True,
         mirror=True),
]
BY_NAME = {c.name: c for c in CASES}

# Distances to the float64 oracle as tests/test_gpu_ranker_pairs.py prints them, each as a FRACTION of the project's bound for it
# (loss 1e-5; a gradient tensor 2e-4 max|g| + 1e-6; a running statistic 1e-5, the variance with rtol 1e-5 on top): (loss, worst
# gradient tensor, worst statistic) of the device, then the same three of the float32 run of the oracle.  MI355X, worst over the
# three steps and, for the mirrored cases, the two iterations of the mask test.  Every case, the 320 and 512 wide ones included,
# stays inside the project's bounds as they are: the allowance of 8 times the float32 oracle's distance is never drawn on.
MEASURED: Dict[str, Tuple[float, ...]] = {
    "l1_ld1_c4": (0.002, 0.016, 0.003, 0.002, 0.019, 0.003),
    "spmm_8_vs_16_drop": (0.001, 0.004, 0.019, 0.006, 0.005, 0.011),
    "class16_mean_c256": (0.003, 0.016, 0.004, 0.009, 0.015, 0.004),
    "class32_c48_c96_ld3": (0.002, 0.016, 0.005, 0.002, 0.010, 0.007),
    "wide_cols_both_mean_drop": (0.005, 0.042, 0.004, 0.007, 0.045, 0.004),
    "wide_col_article_only": (0.003, 0.009, 0.004, 0.003, 0.010, 0.004),
    "sixteen_cols_w12": (0.004, 0.008, 0.010, 0.004, 0.008, 0.009),
    "hidden320_l3_drop": (0.003, 0.007, 0.287, 0.007, 0.007, 0.133),
    "l3_ld3_c20_drop": (0.003, 0.009, 0.051, 0.007, 0.004, 0.045),
    "c512": (0.002, 0.006, 0.005, 0.005, 0.003, 0.005),
    "c12_drop": (0.002, 0.006, 0.007, 0.005, 0.008, 0.007),
    "one_workgroup_l3_drop": (0.002, 0.036, 0.055, 0.007, 0.167, 0.182),
}


# ---- the decision functions, restated ------------------------------------------------------------------------------------------
def embed_pair_form(a_dims, b_dims) -> Optional[int]:
    """Lanes per (node, column) of the merged embedding launch, or None: the two single launches (sage.hip)."""
    if max(max(a_dims), max(b_dims)) <= 64:
        return 16
    if max(a_dims) > 64 and max(b_dims) > 64:
        return 64
    return None


def lpr_class(d4: int) -> int:
    return 8 if d4 <= 8 else 16 if d4 <= 16 else 32 if d4 <= 32 else 64 if d4 <= 64 else 0


def spmm_pair_ok(d_a: int, d_b: int) -> bool:
    ca, cb = lpr_class(d_a // 4), lpr_class(d_b // 4)
    return ca != 0 and ca == cb


def bn_pair_ok(c: int) -> bool:
    return 4 <= c <= 256 and c & (c - 1) == 0


def wgrad_supported(k: int, m: int, n1: int, n2: int) -> bool:
    """wgrad.hip: wg_fill — k rows, m = c_out, n1 = c_src, n2 = c_dst."""
    return k > 0 and 0 < m <= 128 and m % 32 == 0 and 0 < n1 <= 512 and 0 <= n2 <= 512 and k * max(m, n1, n2) < 2 ** 31 - 1


def layer_inputs(case: Case) -> List[Tuple[int, int]]:
    """(customer width, article width) going INTO every encoder layer."""
    out, cur = [], case.widths
    for c in case.conv:
        out.append(cur)
        cur = (c, c)
    return out


def expected_launches(case: Case, aux: bool, n_rows: Tuple[int, int] = (54, 300)) -> Dict[str, Tuple[int, int]]:
    """{kind: (merged, single)} of one step.  n_rows (customers, articles of the batch) only enter wgrad's 32-bit bound."""
    L, LD, drop = len(case.conv), case.dec_layers, case.p > 0
    out = {k: [0, 0] for k in KINDS}

    def decide(kind, shares_an_instantiation=True):
        out[kind][0 if (shares_an_instantiation and not aux) else 1] += 1

    decide("EMBED", embed_pair_form(case.cust_dims, case.art_dims) is not None)
    if drop and L > 1:
        decide("PREP_DROPOUT")
    ins = layer_inputs(case)
    for l in range(L):
        if drop and 0 < l < L - 1:
            decide("DROPOUT")
        decide("SPMM_FWD", spmm_pair_ok(*ins[l]))
        if l > 0:
            decide("SPMM_BWD", spmm_pair_ok(*ins[l]))
    decide("BN_FWD", bn_pair_ok(case.C))
    decide("BN_BWD", bn_pair_ok(case.C))
    decide("GATHER_CAT_BWD")
    out["GATHER_CAT_DROPOUT"][0 if (drop and LD > 1) else 1] += 1
    out["LINEAR1_BWD"][0] += 1
    # relation 0 (customer -> article): k = articles, c_src = customer width, c_dst = article width; relation 1 the other way round
    kernel = [wgrad_supported(n_rows[1], case.conv[l], ins[l][0], ins[l][1]) and wgrad_supported(n_rows[0], case.conv[l], ins[l][1], ins[l][0])
              for l in range(L)]
    out["WGRAD"][0] = (1 if any(kernel) else 0) if L <= 2 else sum(kernel)
    out["WGRAD"][1] = L - sum(kernel)
    return {k: (m, s) for k, (m, s) in out.items()}


def admission_failures(case: Case) -> List[str]:
    """What the executor's validation pass (ranker_exec.hip, CHECK mode) or NativeRankerStep.unsupported_reason would decline
    the case for; empty = taken."""
    bad = []
    L, LD = len(case.conv), case.dec_layers
    if not (1 <= L <= MAX_LAYERS and 1 <= LD <= MAX_LAYERS):
        bad.append("layer count")
    if case.aggr not in ("add", "mean"):
        bad.append("aggr")
    if not 0.0 <= case.p < 1.0:
        bad.append("p")
    for dims in (case.cust_dims, case.art_dims):
        if not 1 <= len(dims) <= MAX_COLS or len(dims) > len(CARDS):
            bad.append("column count")
        if any(not 1 <= d <= 4096 for d in dims):
            bad.append("column width")
    for w_c, w_a in layer_inputs(case):
        if w_c % 4 or w_a % 4 or w_c > 512 or w_a > 512:     # spmm: d % 4 == 0 and d <= 512; conv: c_src, c_dst multiples of 4
            bad.append(f"layer input widths {w_c}, {w_a}")
    if any(c % 4 or not 1 <= c <= 4096 for c in case.conv):
        bad.append("c_out")
    if case.C > 512:
        bad.append("BatchNorm beyond 512 channels")
    # parameters: 3 per conv, 2 relations, 2 BatchNorms of 2, 2 per decoder layer (MI_RANKER_MAX_PARAMS = 48)
    if 6 * L + 4 + 2 * LD > 48:
        bad.append("parameter count")
    return bad


# ---- grids of the launches whose split the table reaches for ---------------------------------------------------------------------
def embed_grid(n: int, n_cols: int, lanes: int) -> int:
    return -(-n * n_cols * lanes // K_BLOCK)


def dropout_grid(n: int, width: int) -> int:
    return -(-(n * width // 4) // K_BLOCK)


# ---- data and models -----------------------------------------------------------------------------------------------------------------
def feature_info(case: Case) -> dict:
    from laplace_amd.data.types import FeatureInfo
    from laplace_amd.utils.constants import Constants
    out = {}
    for key, dims in ((Constants.node_user, case.cust_dims), (Constants.node_item, case.art_dims)):
        out[key] = FeatureInfo(num_feat=len(dims), num_cat=[CARDS[i] - 1 for i in range(len(dims))], embedding_size=list(dims))
    return out


def make_batches(case: Case, n: int = 3, seed: int = 0):
    """n host batches of the case's graph: HeteroData on the CPU.  isolated: one edgeless node of each type is appended."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import GraphDataset
    from laplace_amd.hetero import DataLoader
    from laplace_amd.utils.constants import Constants
    spec = S.SyntheticSpec(400, 120, 3000, seed=seed + 5, deg_min=2, deg_max=60)
    graph, users, articles = S.generate_hetero(spec, customer_cards=CARDS[:len(case.cust_dims)], article_cards=CARDS[:len(case.art_dims)])
    cfg = SimpleNamespace(k=12, num_neighbors=2 if case.small_batch else 8, n_hop_neighbors=2, positive_edges_ratio=0.5,
                          negative_edges_ratio=3.0, batch_size=1 if case.small_batch else 6)
    ds = GraphDataset(cfg, graph, users, articles, train=True, randomization=True, seed=seed)
    loader = DataLoader(ds, batch_size=cfg.batch_size, shuffle=True, generator=t.Generator().manual_seed(seed))
    batches = [b for _, b in zip(range(n), loader)]
    if case.isolated:
        for b in batches:
            for key in (Constants.node_user, Constants.node_item):
                b[key].x = t.cat([b[key].x, b[key].x[:1]], dim=0)
    return batches


def batch_shape(batch) -> dict:
    """Node, edge and label counts of a batch and the in-degrees of both sides of the `buys` relation (from the edge list the
    CSRs are sorted from)."""
    from laplace_amd.utils.constants import Constants
    from laplace_amd.utils.get_info import select_properties
    x, ei, eli, y = select_properties(batch)
    e = next(v for k, v in ei.items() if tuple(k) == tuple(Constants.edge_key))
    n_c, n_a = int(x[Constants.node_user].shape[0]), int(x[Constants.node_item].shape[0])
    return dict(n_c=n_c, n_a=n_a, nnz=int(e.shape[1]), n_label=int(y.numel()),
                deg_c=t.bincount(e[0], minlength=n_c), deg_a=t.bincount(e[1], minlength=n_a))


def make_model(case: Case, first, device, seed: int = 0):
    """Encoder_Decoder_Model of the case on `device`, its lazy layers sized on `first` (a batch on that device)."""
    from laplace_amd.model.encoder_decoder import Encoder_Decoder_Model
    from laplace_amd.model.layers import SAGEConv, get_linear_layers
    t.manual_seed(seed)
    enc = t.nn.ModuleList([SAGEConv((-1, -1, -1), c, aggr=case.aggr, normalize=False, bias=True) for c in case.conv])
    dec = get_linear_layers(case.dec_layers, 2 * case.C, case.dec_hidden, 1)
    model = Encoder_Decoder_Model(encoder_layers=enc, decoder_layers=dec, feature_info=feature_info(case), metadata=first.metadata(),
                                  embedding=True, heterogeneous_prop_agg_type="sum", batch_normalize=True, p_dropout_edges=0.0,
                                  p_dropout_features=case.p).to(device)
    model.initialize_encoder_input_size(first)
    return model
