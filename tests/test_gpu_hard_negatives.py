"""GPU: hard negatives from random-walk ranks (pinsage_hard_neg_kernel through mi_pinsage_hard_negatives and
mi_pinsage_sample_batch_hard) against the CPU mirror of the rule (tests/hard_negatives_emulation.py) bit for bit; the
device-built batches against the index-op path; share 0 / no hard negatives against today's sampler; the overlapped iterator;
one native training iteration on a hard batch."""
import functools
from collections import Counter

import numpy as np
import pytest
import torch as t

import hard_negatives_emulation as HE
from test_gpu_pinsage_device import _graph as _dev_graph
from test_pinsage import _graph

pytestmark = pytest.mark.gpu

SEED = 77
CONFIGS = [(8, 1, 0.0, 0, 1, 1.0),               # the single most-visited item
           (100, 2, 0.5, 3, 10, 0.5),            # mixed selection
           (512, 8, 0.25, 20, 10 ** 6, 1.0),     # 4096 slots, the limit; every window truncated
           (33, 3, 0.5, 30, 40, 1.0),            # 99 slots, not a power of two
           (16, 2, 0.5, 12, 20, 1.0)]


@functools.lru_cache(maxsize=None)
def _g():
    return _graph(seed=2, U=300, I=150, E=3000)


@functools.lru_cache(maxsize=None)
def _mirror(cfg, step):
    """The mirror's 256 pairs of (cfg, step), computed once; pair b does not depend on the batch size, so the batches of 1 and
    37 are its prefixes."""
    users, items, ucsr, icsr, U, I = _g()
    return HE.hard_item_pairs(256, I, icsr, ucsr, HE.Rule(*cfg), SEED, step)


def _hard(cfg):
    from laplace_amd.pinsage.sampler import HardNegatives
    W, L, p, lo, hi, share = cfg
    return HardNegatives(W, L, p, lo, hi, share)


def test_the_mirror_case_is_not_vacuous():
    what = _mirror((33, 3, 0.5, 30, 40, 1.0), 5)[4]
    c = Counter(what)
    print("full / truncated / fall-back:", c["full"], c["truncated"], c["fallback"])
    assert c["full"] >= 10 and c["truncated"] >= 10 and c["fallback"] >= 1


@pytest.mark.parametrize("cfg", CONFIGS)
def test_item_pairs_and_ranks_bit_exact_vs_mirror(cfg):
    from laplace_amd.pinsage.sampler import PinSAGESampler
    users, items, ucsr, icsr, U, I = _g()
    for B in (1, 37, 256):
        smp = PinSAGESampler(users, items, U, I, batch_size=B, seed=SEED, hard_negatives=_hard(cfg))
        for step in (0, 5):
            wh, wt, wn, wr, _ = (x[:B] for x in _mirror(cfg, step))
            keep = wt != -1
            h, tl, ng = smp.item_pairs(step)
            ranks = smp.hard_negative_ranks(step)
            assert ranks.dtype == t.int32 and ranks.shape == (B,)
            assert np.array_equal(h.cpu().numpy(), wh[keep]) and np.array_equal(tl.cpu().numpy(), wt[keep]), (B, step)
            assert np.array_equal(ng.cpu().numpy(), wn[keep]), (B, step)
            assert np.array_equal(ranks.cpu().numpy(), wr), (B, step)


def _hand_graph():
    """10 items, 6 users.  Item 9 has no users (a head 9 is a dead pair); item 8's only user owns only item 8 (walks from 8
    see nothing but 8: m = 0); the rest is small and dense enough for ties among the visit counts."""
    from laplace_amd.data.dataset import AdjList
    from oracle import pinsage_ref as PR
    own = {0: [0, 1, 2, 3], 1: [1, 2, 4], 2: [3, 4, 5, 6], 3: [0, 5, 7], 4: [2, 6, 7], 5: [8]}
    u = np.array([k for k, v in own.items() for _ in v])
    a = np.array([i for v in own.values() for i in v])
    U, I = 6, 10
    users, items = AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, I)
    return users, items, PR.Csr(users.ptr, users.idx), PR.Csr(items.ptr, items.idx), U, I


def test_hand_built_graph():
    from laplace_amd.pinsage.sampler import PinSAGESampler
    users, items, ucsr, icsr, U, I = _hand_graph()
    B, cfg = 48, (8, 2, 0.5, 0, 4, 1.0)
    rule = HE.Rule(*cfg)
    smp = PinSAGESampler(users, items, U, I, batch_size=B, seed=SEED, hard_negatives=_hard(cfg))
    seen_tie = False
    for step in (0, 1):
        wh, wt, wn, wr, what = HE.hard_item_pairs(B, I, icsr, ucsr, rule, SEED, step)
        # what the graph was built for, on the mirror's own output
        dead = [b for b in range(B) if wh[b] == 9]
        lone = [b for b in range(B) if wh[b] == 8]
        assert dead and all(what[b] == "dead" and wr[b] == -1 for b in dead)
        assert lone and all(what[b] == "fallback" and wr[b] == -1 and wt[b] == 8 for b in lone)   # m = 0
        hard_heads = Counter(int(wh[b]) for b in range(B) if wr[b] >= 0)
        assert max(hard_heads.values()) >= 2                                                     # a head drawn twice
        for b in range(B):
            if wr[b] < 0:
                continue
            order = HE.ranked(HE.walk_counts(int(wh[b]), icsr, ucsr, rule, SEED, step), int(wh[b]), int(wt[b]))
            r = int(wr[b])
            if r + 1 < len(order) and order[r + 1][1] == order[r][1]:      # the pick is the lower id of two tied items
                assert order[r][0] < order[r + 1][0]
                seen_tie = True
        # the device against the mirror, dead pairs included
        heads, tails, negs = smp._item_pairs_full(step)
        assert np.array_equal(heads.cpu().numpy(), wh) and np.array_equal(tails.cpu().numpy(), wt)
        assert np.array_equal(negs.cpu().numpy(), wn), step
        assert np.array_equal(smp.hard_negative_ranks(step).cpu().numpy(), wr), step
        keep = wt != -1
        assert all(np.array_equal(x.cpu().numpy(), y[keep]) for x, y in zip(smp.item_pairs(step), (wh, wt, wn)))
    assert seen_tie


def _flat(batch):
    return [batch["seeds"], *batch["pos"], *batch["neg"]] + [x for blk in batch["blocks"] for x in (
        blk["src_ids"], blk["edge_src"], blk["edge_dst"], blk["weights"], blk["csr"][0].rowptr, blk["csr"][0].col, blk["csr"][0].val,
        blk["csr"][1].rowptr, blk["csr"][1].col, blk["csr"][1].val)]


@pytest.mark.parametrize("B", [32, 200])
def test_device_batches_equal_the_index_op_path(B):
    from laplace_amd.pinsage.model import block_csr
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I = 2000, 700
    users, items = _dev_graph(7, U, I, 30000)
    smp = PinSAGESampler(users, items, U, I, batch_size=B, seed=11, hard_negatives=_hard((100, 2, 0.5, 3, 10, 0.5)))
    plain = PinSAGESampler(users, items, U, I, batch_size=B, seed=11)
    for step in (0, 3):
        smp.device_batches = True
        got = smp._sample_batch_device(step)
        assert got is not None
        smp.device_batches = False
        want = smp.sample_batch(step)
        assert bool((smp._pos32 == -1).all())
        assert t.equal(got["seeds"], want["seeds"])
        for a, b in zip(got["pos"] + got["neg"], want["pos"] + want["neg"]):
            assert t.equal(a, b)
        assert len(got["blocks"]) == len(want["blocks"]) == 2
        for gb, wb in zip(got["blocks"], want["blocks"]):
            assert gb["n_dst"] == wb["n_dst"]
            for key in ("src_ids", "edge_src", "edge_dst", "weights"):
                assert t.equal(gb[key], wb[key]), key
            for mine, ref in zip(gb["csr"], block_csr(wb)):
                assert mine.n_rows == ref.n_rows and mine.n_cols == ref.n_cols
                assert t.equal(mine.rowptr, ref.rowptr) and t.equal(mine.col, ref.col) and t.equal(mine.val, ref.val)
        # hard negatives did change the batch: the negatives are not the uniform sampler's
        ranks = smp.hard_negative_ranks(step)
        assert int((ranks >= 0).sum()) > 0
        uni = plain._sample_batch_device(step)
        assert not t.equal(got["seeds"][got["neg"][1]], uni["seeds"][uni["neg"][1]])


def test_share_zero_is_todays_sampler():
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I = 2000, 700
    users, items = _dev_graph(7, U, I, 30000)
    mk = lambda **kw: PinSAGESampler(users, items, U, I, batch_size=64, seed=11, **kw)
    a, b, c = mk(), mk(hard_negatives=None), mk(hard_negatives=_hard((100, 2, 0.5, 3, 10, 0.0)))
    for step in (0, 4):
        ba, bb, bc = (s.sample_batch(step) for s in (a, b, c))
        for x, y, z in zip(_flat(ba), _flat(bb), _flat(bc)):
            assert t.equal(x, y) and t.equal(x, z)
        for x, y, z in zip(a.item_pairs(step), b.item_pairs(step), c.item_pairs(step)):
            assert t.equal(x, y) and t.equal(x, z)
        assert bool((c.hard_negative_ranks(step) == -1).all()) and bool((a.hard_negative_ranks(step) == -1).all())
    c.hard_negatives.share = 1.0                      # read at every launch: the same sampler now gives hard batches
    assert int((c.hard_negative_ranks(0) >= 0).sum()) > 0
    assert not t.equal(c.item_pairs(0)[2], a.item_pairs(0)[2])


def test_overlapped_batches_are_the_serial_batches():
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I = 3000, 900
    users, items = _dev_graph(9, U, I, 50000)
    mk = lambda: PinSAGESampler(users, items, U, I, batch_size=48, seed=21, hard_negatives=_hard((100, 2, 0.5, 3, 10, 0.5)))
    a, b, c = mk(), mk(), mk()
    serial = [a.sample_batch() for _ in range(5)]
    busy = t.randn(2048, 2048, device="cuda")
    prev = None
    for i, batch in enumerate(b.batches(5)):
        if prev is not None:      # the previous batch was not touched by the sampling of this one or of the one in flight
            for x, y in zip(_flat(prev), _flat(serial[i - 1])):
                assert t.equal(x, y), i
        for _ in range(3):
            busy = busy @ busy * 1e-3
        for x, y in zip(_flat(batch), _flat(serial[i])):
            assert x.shape == y.shape and t.equal(x, y), i
        prev = batch
    assert b.step == a.step == 5
    t.cuda.synchronize()
    assert bool((b._pos32 == -1).all()) and all(bool((p == -1).all()) for p in b._lane_pos)
    second = [[x.clone() for x in _flat(batch)] for batch in c.batches(5)]      # two runs give equal bits
    for got, want in zip(second, serial):
        for x, y in zip(got, _flat(want)):
            assert t.equal(x, y)


def test_one_native_iteration_on_a_hard_batch():
    """NativePinSAGEStep takes a batch with hard negatives as it takes any other (one negative per pair, the pair's own head):
    the loss is the autograd iteration's on the same batch, to the tolerance of tests/test_gpu_pinsage_device.py."""
    import copy
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler
    seed, U, I = 2, 2500, 800
    users, items = _dev_graph(seed + 3, U, I, 40000)
    smp = PinSAGESampler(users, items, U, I, batch_size=48, num_layers=2, seed=seed + 1,
                         hard_negatives=_hard((100, 2, 0.5, 3, 10, 0.5)))
    t.manual_seed(seed)
    model = PinSAGEModel(I, 32, 2).to("cuda")
    with t.no_grad():
        model.bias.normal_(0, 0.1)
    for cv in model.convs:
        cv.dropout.p = 0.0
    twin = copy.deepcopy(model)
    opt = t.optim.Adam(model.parameters(), lr=3e-3)
    assert NativePinSAGEStep.unsupported_reason(model, opt) is None
    probe = NativePinSAGEStep(model, opt, keep_grads=True)
    model.train(); twin.train()
    assert int((smp.hard_negative_ranks(smp.step) >= 0).sum()) > 0
    b = smp.sample_batch()
    la = probe.step(b)
    assert la is not None and probe.declined is None, probe.declined
    lb = twin(b["seeds"], b["pos"], b["neg"], b["blocks"]).mean()
    assert abs(float(la) - float(lb)) <= 1e-6 * max(1.0, abs(float(lb)))
