"""A float64 reference, hand-built batches, error bounds and the case table for the native PinSAGE iteration
(csrc/pinsage_exec.hip, mi_pinsage_step_f32) and the item pass (csrc/pinsage_infer.hip) — written from the reference's
pinsage/layers.py:121-156 and pinsage/model.py:16-34 in ordinary torch on the CPU: no laplace_amd op, no kernel, no block_csr.

Shared by tests/test_pinsage_step_refs_cpu.py (the reference, the guard and the bounds are sound; wrong variants of the
reference are refused) and tests/test_gpu_pinsage_step_float64.py (the executor against the reference).

The tolerance of a compared tensor is bound(x64, x32) = 8 max|x32 - x64| + 4 * 2^-24 max|x64|: x32 is THIS file's formulas
evaluated in float32 on the CPU, so the first term is the error of an honest float32 evaluation of the same mathematics (the
factor 8: another, equally valid, summation order — MFMA tiles, split-K slices, wave butterflies); the second is a few ulps of
the tensor's scale for tensors the float32 evaluation happens to get exactly.  Nothing here was fitted to a kernel's output.
"""
import numpy as np
import torch as t

from oracle.philox import philox4x32

U = 2.0 ** -24
MAX_LAYERS = 4            # MI_PINSAGE_MAX_LAYERS (include/laplace_hip.h); the GPU file asserts it against _lib
EXEC_SEED = 0x9E3779B97F4A7C15      # the executor's Philox seed in the dropout cases: both words non-zero


# ----------------------------------------------------------------------------------------------------------- dropout masks
def dropout_threshold(p):
    """The executor's keep threshold: uint32(min(4294967040, float32(p) * 2^32)) (the product is exact: a power of two)."""
    return int(min(4294967040.0, float(np.float32(p)) * 4294967296.0))


def dropout_scale(p):
    """float32(1) / (float32(1) - float32(p)), as a Python float holding that float32 value."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def dropout_mask(seed, iteration, p, site, shape):
    """The 0/1 mask (float64 numpy, `shape` = (rows, cols), cols % 4 == 0) of one launch site: float4 number i of the flat
    matrix takes the four words of philox(counter = (i lo, i hi, site, iteration), key = (seed lo, seed hi)); an element is kept
    when its word is >= the threshold."""
    rows, cols = shape
    assert cols % 4 == 0
    i = np.arange(rows * cols // 4, dtype=np.uint64)
    words = philox4x32(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), site, int(iteration) & 0xFFFFFFFF,
                       int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = np.stack(words, 1).reshape(rows, cols)
    return (w >= np.uint64(dropout_threshold(p))).astype(np.float64)


def dropout_masks(seed, iteration, p, shapes):
    """One mask per site, sites numbered by position: shapes[2 l] = (n_src_l, H), the input of Q_l; shapes[2 l + 1] =
    (n_dst_l, 2 H), the concatenation."""
    return [dropout_mask(seed, iteration, p, site, shape) for site, shape in enumerate(shapes)]


def site_shapes(batch, hidden):
    out = []
    for b in batch["blocks"]:
        out += [(int(b["src_ids"].numel()), hidden), (int(b["n_dst"]), 2 * hidden)]
    return out


class _Drop(t.autograd.Function):
    """y = x * fwd (forward), dx = dy * bwd (backward): the same array twice is dropout; two arrays are a backward that
    regenerated another mask than the forward's."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.save_for_backward(bwd)
        return x * fwd

    @staticmethod
    def backward(ctx, g):
        (bwd,) = ctx.saved_tensors
        return g * bwd, None, None


# --------------------------------------------------------------------------------------------------------------- reference
WRONG = ("n_seeds_mean", "no_final_term", "cat_mask_site", "norm_no_projection", "no_clamp", "second_wave_ignored",
         "margin0_dead", "norm_no_mask")


def reference_step(params, batch, dtype, masks=None, scale=1.0, wrong=None, bwd_masks=None):
    """One PinSAGE training iteration up to the gradients, on the CPU in `dtype`.

    params: {"proj": [n_items + 1, H], "bias": [n_items, 1], "layers": [(Q.weight, Q.bias, W.weight, W.bias), ...]} float32.
    masks: None, or one 0/1 array per site (dropout_masks), multiplied in with `scale`.
    wrong: None for the reference; a name from WRONG for a deliberately wrong variant (test_pinsage_step_refs_cpu.py shows that
    the bounds refuse each); bwd_masks: with "cat_mask_site", the masks the backward takes.
    Returns {"loss", "grads": {"proj", "bias", "Q{l}.weight", "Q{l}.bias", "W{l}.weight", "W{l}.bias"}, "pre": [every relu
    pre-activation, layer by layer: Q's then W's], "margin", "hf"} as float64 tensors of `dtype`'s values."""
    assert wrong is None or wrong in WRONG
    leaf = lambda x: x.detach().to(dtype).clone().requires_grad_(True)
    proj, bias = leaf(params["proj"]), leaf(params["bias"])
    layers = [tuple(leaf(x) for x in lay) for lay in params["layers"]]
    blocks = batch["blocks"]
    seeds, (pu, pv), (_, nv) = batch["seeds"], batch["pos"], batch["neg"]
    n_pairs = int(pu.numel())

    def drop(x, site):
        if masks is None:
            return x
        fwd = t.as_tensor(masks[site]).to(dtype) * t.tensor(scale, dtype=dtype)
        bwd = fwd if bwd_masks is None else t.as_tensor(bwd_masks[site]).to(dtype) * t.tensor(scale, dtype=dtype)
        return _Drop.apply(x, fwd, bwd)

    h = proj[blocks[0]["src_ids"]]
    last = blocks[-1]
    h_dst_final = proj[last["src_ids"][: last["n_dst"]]]
    if wrong == "no_final_term":
        h_dst_final = h_dst_final.detach()
    pre = []
    for l, (blk, (qw, qb, ww, wb)) in enumerate(zip(blocks, layers)):
        n_dst, es, ed = int(blk["n_dst"]), blk["edge_src"], blk["edge_dst"]
        w = blk["weights"].to(dtype)
        h_dst = h[:n_dst]
        n_pre = drop(h, 2 * l) @ qw.T + qb
        n = t.relu(n_pre)
        wsum = t.zeros(n_dst, dtype=dtype).index_add_(0, ed, w)
        wsum = t.where(wsum == 0, t.ones_like(wsum), wsum) if wrong == "no_clamp" else wsum.clamp(min=1)
        agg = t.zeros(n_dst, n.shape[1], dtype=dtype).index_add_(0, ed, n[es] * (w / wsum[ed])[:, None])
        z_pre = drop(t.cat([agg, h_dst], 1), 2 * l + 1) @ ww.T + wb
        z = t.relu(z_pre)
        if wrong == "norm_no_mask":       # the relu applied to the values only: its backward mask is lost
            z = z_pre + (z - z_pre).detach()
        norm = z.norm(2, 1, keepdim=True)
        norm = t.where(norm == 0, t.ones_like(norm), norm)
        h = z / (norm.detach() if wrong == "norm_no_projection" else norm)
        pre += [n_pre, z_pre]
    hf = h_dst_final + h
    score = lambda a, b: (hf[a] * hf[b]).sum(1, keepdim=True) + bias[seeds[a]] + bias[seeds[b]]
    margin = score(pu, nv) - score(pu, pv) + 1
    hinge = t.where(margin > 0, margin, t.zeros_like(margin)) if wrong == "margin0_dead" else margin.clamp(min=0)
    loss = hinge.sum() / (int(seeds.numel()) if wrong == "n_seeds_mean" else n_pairs)
    if wrong == "second_wave_ignored":
        sel = ((t.arange(n_pairs) % 128) < 64).to(dtype)[:, None]
        ((hinge * sel).sum() / n_pairs).backward()
    else:
        loss.backward()
    zero = lambda x: t.zeros_like(x) if x.grad is None else x.grad
    grads = {"proj": zero(proj), "bias": zero(bias)}
    for l, lay in enumerate(layers):
        for name, x in zip(("Q%d.weight", "Q%d.bias", "W%d.weight", "W%d.bias"), lay):
            grads[name % l] = zero(x)
    d = lambda x: x.detach().double()
    return {"loss": d(loss), "grads": {k: d(v) for k, v in grads.items()}, "pre": [d(x) for x in pre], "margin": d(margin),
            "hf": d(hf)}


def reference_forward(params, blocks, dtype):
    """get_repr in eval mode (no dropout, no pairs): h_dst_final + h over `blocks`, and the relu pre-activations."""
    cast = lambda x: x.detach().to(dtype)
    proj = cast(params["proj"])
    h = proj[blocks[0]["src_ids"]]
    last = blocks[-1]
    h_dst_final = proj[last["src_ids"][: last["n_dst"]]]
    pre = []
    for blk, lay in zip(blocks, params["layers"]):
        qw, qb, ww, wb = (cast(x) for x in lay)
        n_dst, es, ed = int(blk["n_dst"]), blk["edge_src"], blk["edge_dst"]
        w = blk["weights"].to(dtype)
        n_pre = h @ qw.T + qb
        n = t.relu(n_pre)
        wsum = t.zeros(n_dst, dtype=dtype).index_add_(0, ed, w).clamp(min=1)
        agg = t.zeros(n_dst, n.shape[1], dtype=dtype).index_add_(0, ed, n[es] * (w / wsum[ed])[:, None])
        z_pre = t.cat([agg, h[:n_dst]], 1) @ ww.T + wb
        z = t.relu(z_pre)
        norm = z.norm(2, 1, keepdim=True)
        norm = t.where(norm == 0, t.ones_like(norm), norm)
        h = z / norm
        pre += [n_pre.double(), z_pre.double()]
    return (h_dst_final + h).double(), pre


# --------------------------------------------------------------------------------------------------------- bound and guard
def bound(x64, x32):
    x64, x32 = t.as_tensor(x64).double(), t.as_tensor(x32).double()
    return 8.0 * float((x32 - x64).abs().max()) + 4.0 * U * float(x64.abs().max())


def structural_zero(x64, x32):
    """A tensor the case makes exactly zero (both evaluations give 0 everywhere — the Q gradients of a block without edges,
    every gradient of a batch without a live pair): compared with ==, not with bound()."""
    return float(t.as_tensor(x64).abs().max()) == 0.0 and float(t.as_tensor(x32).abs().max()) == 0.0


def guard(pre64, pre32, margin64, margin32):
    """Whether a float32 evaluation can be compared with the float64 one at all: at every relu site and for the margins,
    |x64| >= 32 max|x32 - x64| (the maximum over that site), so that no honest float32 evaluation lands on the other side of
    a kink.  Entries that are <= 0 in float64 and bitwise the same in float32 are exempt: constants of the construction (a
    bias of -1, a structural 0).  Returns (ok, the smallest |x64| / (32 max err) over the sites: the margin of safety)."""
    worst = float("inf")
    for a, b in list(zip(pre64, pre32)) + [(margin64, margin32)]:
        a, b = a.double(), b.double()
        err = float((a - b).abs().max())
        live = ~((a <= 0) & (a == b))
        if err == 0.0 or not bool(live.any()):
            continue
        worst = min(worst, float(a[live].abs().min()) / (32.0 * err))
    return worst >= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ batches
def make_params(gen, n_items, hidden, n_layers):
    """Table randn * 0.5, Q / W weights randn / sqrt(fan-in), layer biases and the scorer bias randn * 0.1 (float32)."""
    rn = lambda *s: t.randn(*s, generator=gen)
    layers = [(rn(hidden, hidden) / hidden ** 0.5, rn(hidden) * 0.1, rn(hidden, 2 * hidden) / (2 * hidden) ** 0.5, rn(hidden) * 0.1)
              for _ in range(n_layers)]
    return {"proj": rn(n_items + 1, hidden) * 0.5, "bias": rn(n_items, 1) * 0.1, "layers": layers}


def make_item_params(gen, n_items, hidden, n_layers):
    """Parameters for the item pass.  A whole catalogue puts 10^5 relu pre-activations at stake at once, and with make_params'
    scales a few of them always land within 32 float32 errors of 0, whatever the seed.  Here the layer biases keep away from 0
    (a random sign times 0.5 .. 1) and the weights are a quarter of make_params', so a pre-activation is its bias plus a term
    of standard deviation ~0.1: both signs occur in every layer, and guard() is passable."""
    P = make_params(gen, n_items, hidden, n_layers)
    gap = lambda: (t.randint(0, 2, (hidden,), generator=gen) * 2 - 1).float() * (0.5 + 0.5 * t.rand(hidden, generator=gen))
    P["layers"] = [(qw * 0.25, gap(), ww * 0.25, gap()) for qw, qb, ww, wb in P["layers"]]
    return P


def make_blocks(gen, n_items, seeds, n_layers, degree=3, weights="counts", src_from_dst=(), pad_src0=None, hub=None,
                isolated=()):
    """Blocks in the sampler's layout, built from the seeds outwards as the sampler does: a block's destinations are the
    first n_dst of its src_ids, its new sources follow in order of first appearance; block l's destinations are block
    l + 1's sources.  Returned input layer first.

    degree: in-edges per destination — an int, or f(depth, n_dst) -> int64[n_dst] (depth 0 = the block around the seeds).
    weights: "counts" (integers 1 .. 5, as visit counts are) or "fractions" (0.25 / 0.5 with every destination's sum < 1).
    src_from_dst: depths whose sources are drawn among the block's own destinations (n_src == n_dst).
    pad_src0: the input block is given further sources, one edge each, until it has exactly this many.
    hub: (depth, item id): one more edge from that item into every destination of that block.
    isolated: item ids that get no in-edge and are nobody's source in any block."""
    ri = lambda hi, n: t.randint(0, hi, (n,), generator=gen)
    iso = set(int(x) for x in isolated)
    dst_ids = [int(x) for x in seeds]
    blocks = []
    for depth in range(n_layers):
        n_dst = len(dst_ids)
        deg = degree(depth, n_dst) if callable(degree) else t.full((n_dst,), int(degree), dtype=t.int64)
        pos = {g: i for i, g in enumerate(dst_ids)}
        src_ids = list(dst_ids)
        es, ed, ew = [], [], []

        def edge(g, d, w):
            if g not in pos:
                pos[g] = len(src_ids)
                src_ids.append(g)
            es.append(pos[g]); ed.append(d); ew.append(w)

        for d in range(n_dst):
            k = 0 if dst_ids[d] in iso else int(deg[d])
            chosen = set()
            while len(chosen) < k:
                g = dst_ids[int(ri(n_dst, 1))] if depth in src_from_dst else int(ri(n_items, 1))
                if g in iso or g in chosen or (hub and g == hub[1]):
                    continue
                chosen.add(g)
                if weights == "counts":
                    w = float(1 + int(ri(5, 1)))
                else:
                    w = 0.5 if (k <= 2 and len(chosen) == 1 and int(ri(2, 1))) else 0.25
                edge(g, d, w)
            if hub and hub[0] == depth and dst_ids[d] not in iso:
                edge(int(hub[1]), d, 0.25 if weights == "fractions" else 2.0)
        if pad_src0 is not None and depth == n_layers - 1:
            assert len(src_ids) <= pad_src0
            while len(src_ids) < pad_src0:
                g = int(ri(n_items, 1))
                if g not in pos and g not in iso:
                    edge(g, int(ri(n_dst, 1)), float(1 + int(ri(5, 1))))
        blocks.insert(0, {"src_ids": t.tensor(src_ids, dtype=t.int64), "n_dst": n_dst,
                          "edge_src": t.tensor(es, dtype=t.int64), "edge_dst": t.tensor(ed, dtype=t.int64),
                          "weights": t.tensor(ew, dtype=t.float32)})
        dst_ids = src_ids
    assert len(set(dst_ids)) == len(dst_ids)
    return blocks


def make_pairs(gen, n_seeds, n_pairs, kind="ordinary"):
    """(u, v, w) int64[n_pairs]: indices into the seeds, three different seeds per pair (one seed: all 0).  "hub": seed 0 is
    an end of every pair — head, tail and negative in turn — the other two ends drawn among the other seeds."""
    if n_seeds == 1:
        z = t.zeros(n_pairs, dtype=t.int64)
        return z, z.clone(), z.clone()
    lo = 1 if kind == "hub" else 0
    m = n_seeds - lo
    assert m >= 3
    u = t.randint(0, m, (n_pairs,), generator=gen)
    v = (u + 1 + t.randint(0, m - 1, (n_pairs,), generator=gen)) % m
    w = t.randint(0, m, (n_pairs,), generator=gen)
    for _ in range(200):
        bad = (w == u) | (w == v)
        if not bool(bad.any()):
            break
        w[bad] = t.randint(0, m, (int(bad.sum()),), generator=gen)
    assert not bool(((w == u) | (w == v)).any())
    u, v, w = u + lo, v + lo, w + lo
    if kind == "hub":
        k = t.arange(n_pairs) % 3
        u[k == 0], v[k == 1], w[k == 2] = 0, 0, 0
    return u, v, w


def make_batch(seeds, blocks, pairs):
    """The batch dict NativePinSAGEStep._prepare reads: neg[0] IS pos[0]; the blocks come without "csr"."""
    u, v, w = (x.to(t.int64).contiguous() for x in pairs)
    assert int(blocks[-1]["n_dst"]) == int(t.as_tensor(seeds).numel())
    return {"seeds": t.as_tensor(seeds, dtype=t.int64).clone(), "pos": (u, v), "neg": (u, w), "blocks": blocks}


def batch_to(batch, device):
    """A copy on `device` that keeps the layout's identities (neg[0] is pos[0])."""
    u, v, w = batch["pos"][0].to(device), batch["pos"][1].to(device), batch["neg"][1].to(device)
    blocks = [{k: (x.to(device) if isinstance(x, t.Tensor) else x) for k, x in b.items() if k != "csr"} for b in batch["blocks"]]
    return {"seeds": batch["seeds"].to(device), "pos": (u, v), "neg": (u, w), "blocks": blocks}


# ----------------------------------------------------------------------------------------------------------------- the cases
# name -> (options of build_case, data seed).  A seed is moved on when the data fail guard() (tools: the CPU file's first
# test names the failing case); none of them was chosen by looking at a kernel's output.
def _c(seed=0, **kw):
    return kw, seed


_DEG_HUB16 = lambda depth, n: t.tensor([0, 16, 0] + [3] * (n - 3), dtype=t.int64)[:n]

CASES = {}
for _h in (4, 8, 12, 20, 68, 100, 124, 128):
    CASES["A-h%d" % _h] = _c(hidden=_h)
for _n in (1, 63, 64, 65, 128, 129):
    CASES["B-p%d" % _n] = _c(n_seeds=5, n_pairs=_n)
for _n in (300, 1024):
    CASES["B-p%d" % _n] = _c(n_seeds=5, n_pairs=_n, pairs="hub")
CASES["C-i"] = _c(n_pairs=64, pairs="tail_is_negative", exact="zero")
CASES["C-ii"] = _c(pairs="head_is_tail")
CASES["C-iii"] = _c(n_seeds=1, n_pairs=1, exact="zero")
CASES["D"] = _c(pairs="disjoint", special="dead", exact="dead")
CASES["E"] = _c(pairs="disjoint", special="margin0", exact="margin0")
CASES["F-i"] = _c(special="zero_rows")
CASES["F-ii"] = _c(special="zero_rows_paired")
CASES["G-i"] = _c(degree=0)
CASES["G-ii"] = _c(degree=lambda depth, n: t.full((n,), 3 if depth == 0 else 0, dtype=t.int64))
CASES["G-iii"] = _c(src_from_dst=(1,))
CASES["G-iv"] = _c(degree=_DEG_HUB16)
CASES["G-v"] = _c(weights="fractions")
CASES["G-vi"] = _c(n_seeds=300, n_pairs=300, degree=1, hub_all=True, n_items=2000)
CASES["H-511"] = _c(pad_src0=511, n_items=1500)
CASES["H-640"] = _c(pad_src0=640, n_items=1500)
for _l in range(1, MAX_LAYERS + 1):
    CASES["I-L%d" % _l] = _c(n_layers=_l, n_items=300)
for _p in (0.5, 0.25, 0.1):
    for _h in (32, 20):
        CASES["J-p%g-h%d" % (_p, _h)] = _c(p=_p, hidden=_h)
# K: the executor's compact-row mode (rows_out / bias_out) on a sparse_tables model: the data of the case named
K_CASES = ("A-h20", "A-h128", "B-p129", "G-i", "G-iv", "J-p0.5-h32")

SEEDS = {"A-h100": 1, "B-p65": 1, "G-vi": 6, "I-L4": 1}       # case -> data seed, where the seeds before it fail the guard
for _k, _s in SEEDS.items():
    CASES[_k] = (CASES[_k][0], _s)


def build_case(name):
    """{"params", "batch", "p", "hidden", "n_items", "exact", "zero_rows"} of a case of the table (CPU tensors)."""
    o, seed = CASES[name]
    o = dict(o)
    gen = t.Generator().manual_seed(7919 * seed + sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    hidden, n_layers, n_seeds, n_pairs = o.get("hidden", 32), o.get("n_layers", 2), o.get("n_seeds", 9), o.get("n_pairs", 40)
    n_items, special, pairs_kind = o.get("n_items", 64), o.get("special"), o.get("pairs", "ordinary")
    params = make_params(gen, n_items, hidden, n_layers)
    seeds = t.randperm(n_items, generator=gen)[:n_seeds]
    zero_seeds = seeds[:3].tolist() if special in ("zero_rows", "zero_rows_paired") else []
    hub = None
    if o.get("hub_all"):
        hub = (0, int([x for x in range(n_items) if x not in set(seeds.tolist())][0]))
    blocks = make_blocks(gen, n_items, seeds, n_layers, degree=o.get("degree", 3), weights=o.get("weights", "counts"),
                         src_from_dst=o.get("src_from_dst", ()), pad_src0=o.get("pad_src0"), hub=hub, isolated=zero_seeds)
    if pairs_kind == "ordinary":
        pairs = make_pairs(gen, n_seeds, n_pairs)
        if special == "zero_rows":            # the three zero rows stay out of the pairs: their table gradient is exactly 0
            u, v, w = make_pairs(gen, n_seeds - 3, n_pairs)
            pairs = (u + 3, v + 3, w + 3)
    elif pairs_kind == "hub":
        pairs = make_pairs(gen, n_seeds, n_pairs, kind="hub")
    elif pairs_kind == "tail_is_negative":
        u, v, _ = make_pairs(gen, n_seeds, n_pairs)
        pairs = (u, v, v.clone())
    elif pairs_kind == "head_is_tail":
        u, v, w = make_pairs(gen, n_seeds, n_pairs)
        v = t.where(t.arange(n_pairs) % 3 == 0, u, v)
        pairs = (u, v, w)
    elif pairs_kind == "disjoint":            # heads among the first third of the seeds, tails the second, negatives the last
        k = n_seeds // 3
        pairs = tuple(j * k + t.randint(0, k, (n_pairs,), generator=gen) for j in range(3))
    batch = make_batch(seeds, blocks, pairs)
    u, v, w = pairs
    if special == "dead":
        params["bias"][seeds[v]] = 50.0
        params["bias"][seeds[w]] = -50.0
    if special == "margin0":
        params["proj"].zero_()
        params["bias"].zero_()
        params["bias"][seeds[v]] = 1.0
        params["layers"] = [(qw, t.zeros_like(qb), ww, t.full_like(wb, -1.0)) for qw, qb, ww, wb in params["layers"]]
    if zero_seeds:
        params["proj"][zero_seeds] = 0.0
        params["layers"] = [(qw, qb, ww, -0.1 * t.randn(hidden, generator=gen).abs()) for qw, qb, ww, wb in params["layers"]]
    return {"name": name, "params": params, "batch": batch, "p": float(o.get("p", 0.0)), "hidden": hidden, "n_items": n_items,
            "exact": o.get("exact"), "zero_rows": zero_seeds}


_EVAL = {}


def evaluate_case(name, iteration=0):
    """(case, float64 result, float32 result) of a case, with the executor's masks of `iteration` in the dropout cases;
    computed once per (case, iteration) and shared: callers must not modify what they get."""
    key = (name, iteration)
    if key not in _EVAL:
        case = build_case(name)
        masks, scale = None, 1.0
        if case["p"] > 0:
            masks = dropout_masks(EXEC_SEED, iteration, case["p"], site_shapes(case["batch"], case["hidden"]))
            scale = dropout_scale(case["p"])
        r64 = reference_step(case["params"], case["batch"], t.float64, masks, scale)
        r32 = reference_step(case["params"], case["batch"], t.float32, masks, scale)
        _EVAL[key] = (case, r64, r32)
    return _EVAL[key]


def compared(r64, r32):
    """[(name, x64, x32)]: the loss and every gradient."""
    return [("loss", r64["loss"], r32["loss"])] + [(k, r64["grads"][k], r32["grads"][k]) for k in r64["grads"]]
