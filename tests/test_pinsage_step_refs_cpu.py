"""CPU: the float64 reference of the PinSAGE iteration (tests/pinsage_step_refs.py) is sound before a kernel is held against it —
every case's data pass the relu / hinge guard, no bound is trivial, the bounds refuse each of a list of deliberately wrong
variants of the reference, the hand-built batches have the sampler's layout, and the dropout masks are the documented Philox
draws."""
import numpy as np
import pytest
import torch as t

import pinsage_step_refs as R
from oracle.philox import philox4x32

ITERATIONS = lambda name: (0, 1) if name.startswith("J") else (0,)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_passes_the_guard_and_its_bounds_are_not_trivial(name):
    for it in ITERATIONS(name):
        case, r64, r32 = R.evaluate_case(name, it)
        ok, worst = R.guard(r64["pre"], r32["pre"], r64["margin"], r32["margin"])
        assert ok, (name, it, worst)
        assert bool(((r64["margin"] > 0) == (r32["margin"] > 0)).all())
        for a, b in zip(r64["pre"], r32["pre"]):
            assert bool(((a > 0) == (b > 0)).all())
        if case["exact"] in ("zero", "dead"):
            continue
        for key, x64, x32 in R.compared(r64, r32):
            if R.structural_zero(x64, x32):                          # exactly known: compared with ==
                assert case["exact"] == "margin0" or (name in ("G-i", "G-ii") and key.startswith("Q")), (name, key)
                continue
            assert not (case["exact"] == "margin0" and key != "bias"), key
            assert R.bound(x64, x32) > 0.0, (name, key)
            assert float((x32 - x64).abs().max()) <= R.bound(x64, x32)


@pytest.mark.parametrize("name", list(R.CASES))
def test_batch_has_the_sampler_layout(name):
    case = R.build_case(name)
    b, blocks = case["batch"], case["batch"]["blocks"]
    assert b["neg"][0] is b["pos"][0]
    assert len(set(blocks[0]["src_ids"].tolist())) == blocks[0]["src_ids"].numel()
    for l, blk in enumerate(blocks):
        assert "csr" not in blk
        assert blk["src_ids"].dtype == blk["edge_src"].dtype == blk["edge_dst"].dtype == t.int64 and blk["weights"].dtype == t.float32
        n_src, n_dst = blk["src_ids"].numel(), blk["n_dst"]
        assert 1 <= n_dst <= n_src and int(blk["src_ids"].max()) < case["n_items"]
        if blk["edge_src"].numel():
            assert 0 <= int(blk["edge_src"].min()) and int(blk["edge_src"].max()) < n_src
            assert 0 <= int(blk["edge_dst"].min()) and int(blk["edge_dst"].max()) < n_dst
        if l + 1 < len(blocks):
            assert t.equal(blk["src_ids"][:n_dst], blocks[l + 1]["src_ids"])
    assert blocks[-1]["n_dst"] == b["seeds"].numel() and t.equal(blocks[-1]["src_ids"][: b["seeds"].numel()], b["seeds"])
    for x in (*b["pos"], b["neg"][1]):
        assert x.dtype == t.int64 and 0 <= int(x.min()) and int(x.max()) < b["seeds"].numel()


def test_cases_reach_the_branches_they_are_named_for():
    blocks = lambda n: R.build_case(n)["batch"]["blocks"]
    pairs = lambda n: (*R.build_case(n)["batch"]["pos"], R.build_case(n)["batch"]["neg"][1])
    for n in ("B-p300", "B-p1024"):            # seed 0 ends every pair; hits in both wavefronts and in several rounds
        u, v, w = pairs(n)
        assert bool(((u == 0) | (v == 0) | (w == 0)).all())
        active = R.evaluate_case(n)[1]["margin"][:, 0] > 0
        idx = t.nonzero(active)[:, 0]
        assert int(active.sum()) > 128 and bool(((idx % 128) >= 64).any()) and bool(((idx % 128) < 64).any())
    assert int((R.evaluate_case("B-p1024")[1]["margin"] > 0).sum()) > 512
    u, v, w = pairs("C-i")
    assert t.equal(v, w) and u.numel() == 64
    u, v, w = pairs("C-ii")
    assert bool((u == v).any()) and bool((u != v).any())
    assert all(x.tolist() == [0] for x in pairs("C-iii"))
    for n in ("D", "E"):
        u, v, w = (set(x.tolist()) for x in pairs(n))
        assert not (u & v or u & w or v & w)
    assert float(R.evaluate_case("D")[1]["margin"].max()) < 0
    assert bool((R.evaluate_case("E")[1]["margin"] == 0).all()) and bool((R.evaluate_case("E")[2]["margin"] == 0).all())
    assert float(R.evaluate_case("E")[1]["hf"].abs().max()) == 0.0
    for n in ("F-i", "F-ii"):
        case, r64, _ = R.evaluate_case(n)
        assert len(case["zero_rows"]) == 3
        assert float(r64["hf"][:3].abs().max()) == 0.0 and float(r64["hf"][3:].abs().min(1).values.max()) > 0
        for blk in case["batch"]["blocks"]:
            assert not bool((blk["edge_dst"] < 3).any()) and not bool((blk["edge_src"] < 3).any())
        in_pairs = any(bool((x < 3).any()) for x in pairs(n))
        assert in_pairs == (n == "F-ii")
    assert [b["edge_src"].numel() for b in blocks("G-i")] == [0, 0]
    assert blocks("G-ii")[0]["edge_src"].numel() == 0 and blocks("G-ii")[1]["edge_src"].numel() > 0
    b0 = blocks("G-iii")[0]
    assert b0["n_dst"] == b0["src_ids"].numel() and b0["edge_src"].numel() > 0
    for blk in blocks("G-iv"):
        deg = t.bincount(blk["edge_dst"], minlength=blk["n_dst"])
        assert deg[:3].tolist() == [0, 16, 0]
    for blk in blocks("G-v"):
        ws = t.zeros(blk["n_dst"]).index_add_(0, blk["edge_dst"], blk["weights"])
        assert float(ws.max()) < 1.0 and set(blk["weights"].tolist()) <= {0.25, 0.5}
    last = blocks("G-vi")[-1]
    assert last["n_dst"] == 300 and int(t.bincount(last["edge_src"]).max()) == 300
    assert blocks("H-511")[0]["src_ids"].numel() == 511 and blocks("H-640")[0]["src_ids"].numel() == 640
    assert [len(blocks("I-L%d" % l)) for l in range(1, R.MAX_LAYERS + 1)] == list(range(1, R.MAX_LAYERS + 1))


def _refused(name, wrong, iteration=0, bwd_masks=None):
    """Whether the float64 evaluation of the wrong variant leaves bound() on at least one compared tensor of the case."""
    case, r64, r32 = R.evaluate_case(name, iteration)
    masks, scale = None, 1.0
    if case["p"] > 0:
        masks = R.dropout_masks(R.EXEC_SEED, iteration, case["p"], R.site_shapes(case["batch"], case["hidden"]))
        scale = R.dropout_scale(case["p"])
    bad = R.reference_step(case["params"], case["batch"], t.float64, masks, scale, wrong=wrong, bwd_masks=bwd_masks)
    got = dict((k, x) for k, x, _ in R.compared(bad, bad))
    return [k for k, x64, x32 in R.compared(r64, r32) if float((got[k] - x64).abs().max()) > R.bound(x64, x32)]


@pytest.mark.parametrize("wrong,name", [
    ("n_seeds_mean", "A-h20"),               # 1 / n_seeds in place of 1 / n_pairs
    ("no_final_term", "A-h20"),              # the seeds' second table-gradient term (h_dst_final) left out
    ("norm_no_projection", "A-h20"),         # the - h (h . dh) term of the norm's backward left out
    ("no_clamp", "G-v"),                     # weights divided by sum w, not by clamp(sum w, 1)
    ("second_wave_ignored", "B-p129"),       # pairs with (index mod 128) >= 64 ignored in the score gradient
    ("second_wave_ignored", "B-p1024"),
    ("margin0_dead", "E"),                   # margin-0 pairs treated as dead
    ("norm_no_mask", "F-ii"),                # the relu mask in front of the norm lost in the backward (rows of norm 0 included)
])
def test_bounds_refuse_a_wrong_variant(wrong, name):
    assert _refused(name, wrong), (wrong, name)
    assert not _refused(name, None)


@pytest.mark.parametrize("name", ["J-p0.5-h32", "J-p0.1-h20"])
def test_bounds_refuse_misplaced_dropout_masks(name):
    """The concatenation's backward mask taken from site 2 l instead of 2 l + 1; the masks of another iteration."""
    case = R.build_case(name)
    shapes, p = R.site_shapes(case["batch"], case["hidden"]), case["p"]
    for it in (0, 1):
        right = R.dropout_masks(R.EXEC_SEED, it, p, shapes)
        wrong_site = [m if s % 2 == 0 else R.dropout_mask(R.EXEC_SEED, it, p, s - 1, shapes[s]) for s, m in enumerate(right)]
        assert _refused(name, "cat_mask_site", it, wrong_site)
        other_iteration = R.dropout_masks(R.EXEC_SEED, 1 - it, p, shapes)
        assert _refused(name, "cat_mask_site", it, other_iteration)
        assert not _refused(name, "cat_mask_site", it, right)


# ---------------------------------------------------------------------------------------------------------------- the masks
@pytest.mark.parametrize("p", [0.5, 0.25, 0.1])
def test_dropout_keep_rate(p):
    n = 100_000
    m = R.dropout_mask(R.EXEC_SEED, 0, p, 0, (n // 4, 4))
    sd = (p * (1 - p) / n) ** 0.5
    assert abs(m.mean() - (1 - p)) <= 4 * sd
    assert set(np.unique(m)) == {0.0, 1.0}


def test_dropout_masks_differ_by_site_iteration_and_seed_word():
    shape, p = (64, 32), 0.5
    base = R.dropout_mask(R.EXEC_SEED, 0, p, 0, shape)
    assert np.array_equal(base, R.dropout_mask(R.EXEC_SEED, 0, p, 0, shape))
    others = [R.dropout_mask(R.EXEC_SEED, 0, p, 1, shape), R.dropout_mask(R.EXEC_SEED, 1, p, 0, shape),
              R.dropout_mask(R.EXEC_SEED ^ 1, 0, p, 0, shape), R.dropout_mask(R.EXEC_SEED ^ (1 << 32), 0, p, 0, shape)]
    for i, m in enumerate(others):
        assert 0.3 < float((m != base).mean()) < 0.7, i
        for n in others[i + 1:]:
            assert not np.array_equal(m, n)
    assert (R.EXEC_SEED >> 32) != 0 and (R.EXEC_SEED & 0xFFFFFFFF) != 0
    masks = R.dropout_masks(R.EXEC_SEED, 3, p, [(5, 8), (3, 16)])
    assert [m.shape for m in masks] == [(5, 8), (3, 16)]
    assert np.array_equal(masks[1], R.dropout_mask(R.EXEC_SEED, 3, p, 1, (3, 16)))


@pytest.mark.parametrize("p", [0.5, 0.25, 0.1])
def test_vectorised_masks_equal_a_scalar_restatement(p):
    seed, iteration, site, cols = R.EXEC_SEED, 1, 3, 16
    m = R.dropout_mask(seed, iteration, p, site, (8, cols)).reshape(-1)
    thr = np.uint32(min(np.float32(4294967040.0), np.float32(p) * np.float32(4294967296.0)))
    for e in range(64):
        i = e // 4
        words = philox4x32(i & 0xFFFFFFFF, i >> 32, site, iteration, seed & 0xFFFFFFFF, seed >> 32)
        assert m[e] == (1.0 if np.uint32(int(words[e % 4])) >= thr else 0.0), e
    assert R.dropout_scale(p) == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    assert R.dropout_threshold(0.99999999) == 4294967040           # the clamp below 2^32


def test_reference_is_the_documented_mathematics_on_a_case_small_enough_to_write_out():
    """One layer, two seeds, one edge, hidden 4: the loss and d bias from the formulas of pinsage/layers.py written out by hand."""
    H = 4
    g = t.Generator().manual_seed(5)
    params = R.make_params(g, 6, H, 1)
    blocks = [{"src_ids": t.tensor([2, 4, 5]), "n_dst": 2, "edge_src": t.tensor([2]), "edge_dst": t.tensor([0]),
               "weights": t.tensor([0.5])}]
    batch = R.make_batch(t.tensor([2, 4]), blocks, (t.tensor([0]), t.tensor([1]), t.tensor([0])))
    r = R.reference_step(params, batch, t.float64)
    P, (qw, qb, ww, wb) = params["proj"].double(), (x.double() for x in params["layers"][0])
    n5 = t.relu(qw @ P[5] + qb)
    hf = []
    for item, agg in ((2, 0.5 * n5), (4, t.zeros(H, dtype=t.float64))):      # sum w = 0.5 < 1: divided by 1
        z = t.relu(ww @ t.cat([agg, P[item]]) + wb)
        nz = z.norm()
        hf.append(P[item] + z / (nz if nz > 0 else 1.0))
    b = params["bias"].double()[:, 0]
    pos = hf[0] @ hf[1] + b[2] + b[4]
    neg = hf[0] @ hf[0] + b[2] + b[2]
    margin = neg - pos + 1
    assert abs(float(r["margin"]) - float(margin)) <= 1e-14
    assert abs(float(r["loss"]) - max(float(margin), 0.0)) <= 1e-14
    if float(margin) > 0:
        assert float(r["grads"]["bias"][2]) == 1.0 and float(r["grads"]["bias"][4]) == -1.0
