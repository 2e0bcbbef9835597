"""Hard negatives from random-walk ranks (PinSAGE section 3.3) without a GPU: the laws of the CPU mirror of the rule
(tests/hard_negatives_emulation.py), the validation of pinsage.sampler.HardNegatives, and the argument checks of
mi_pinsage_hard_negatives / mi_pinsage_sample_batch_hard (they return before anything touches a device)."""
import ctypes

import numpy as np
import pytest

import hard_negatives_emulation as HE
from oracle import pinsage_ref as PR
from test_pinsage import _graph


@pytest.fixture(scope="module")
def graph():
    return _graph(seed=2, U=300, I=150, E=3000)


def _reachable(h, L, icsr, ucsr):
    """Items reachable from h within L item -> user -> item traversals."""
    seen, frontier = set(), {int(h)}
    for _ in range(L):
        nxt = set()
        for i in frontier:
            for u in icsr[i]:
                nxt.update(int(v) for v in ucsr[int(u)])
        seen |= nxt
        frontier = nxt
    return seen


@pytest.mark.parametrize("cfg", [(16, 2, 0.5, 12, 20, 1.0), (33, 3, 0.5, 30, 40, 1.0), (100, 2, 0.5, 3, 10, 0.5), (8, 1, 0.0, 0, 1, 1.0)])
def test_mirror_laws(graph, cfg):
    users, items, ucsr, icsr, U, I = graph
    rule = HE.Rule(*cfg)
    B, seed, step = 64, 77, 5
    heads, tails, negs, ranks, what = HE.hard_item_pairs(B, I, icsr, ucsr, rule, seed, step)
    uniform = [PR._words(PR.P_NEG, b, 0, 0, seed, step)[0] % I for b in range(B)]
    replaced = 0
    for b in range(B):
        h, tl, ng, r = int(heads[b]), int(tails[b]), int(negs[b]), int(ranks[b])
        if r < 0:
            assert ng == uniform[b] and what[b] in ("dead", "uniform", "fallback")
            assert (tl == -1) == (what[b] == "dead")
            continue
        replaced += 1
        assert ng != h and ng != tl
        assert ng in _reachable(h, rule.walk_length, icsr, ucsr)
        order = HE.ranked(HE.walk_counts(h, icsr, ucsr, rule, seed, step), h, tl)
        m = len(order)
        assert rule.rank_lo <= r < min(rule.rank_hi, m) and order[r][0] == ng
        assert all((order[i][1], -order[i][0]) >= (order[i + 1][1], -order[i + 1][0]) for i in range(m - 1))  # count desc, id asc
        assert what[b] == ("truncated" if m < rule.rank_hi else "full")
    assert replaced > 0


def test_share_zero_is_the_uniform_sampler(graph):
    users, items, ucsr, icsr, U, I = graph
    for step in (0, 5):
        heads, tails, negs, ranks, what = HE.hard_item_pairs(64, I, icsr, ucsr, HE.Rule(16, 2, 0.5, 0, 5, 0.0), 77, step)
        wh, wt, wn = PR.item_pairs(64, I, icsr, ucsr, 77, step)
        keep = tails != -1
        assert np.array_equal(heads[keep], wh) and np.array_equal(tails[keep], wt) and np.array_equal(negs[keep], wn)
        assert (ranks == -1).all() and set(what) <= {"dead", "uniform"}


def test_selection_rate():
    """share = 0.5, batch 256, seed 77, step 5: 128 +/- 4 sigma, sigma = sqrt(256 / 4) = 8.  (The mirror gave 116.)"""
    n = sum(HE.selected(b, 0.5, 77, 5)[0] for b in range(256))
    print("selected pairs:", n)
    assert 96 <= n <= 160
    assert all(HE.selected(b, 1.0, 77, 5)[0] for b in range(256)) and not any(HE.selected(b, 0.0, 77, 5)[0] for b in range(256))


def test_hard_negatives_class_validates():
    from laplace_amd.pinsage.sampler import HardNegatives
    hn = HardNegatives(rank_lo=5, rank_hi=30)
    assert (hn.num_walks, hn.walk_length, hn.restart_prob, hn.share) == (256, 2, 0.5, 1.0)
    s = hn.struct()
    assert (s.num_walks, s.walk_length, s.rank_lo, s.rank_hi, s.restart_prob, s.share) == (256, 2, 5, 30, 0.5, 1.0)
    hn.share = 0.25                                   # the curriculum: reassigned between epochs, read at every launch
    assert hn.struct().share == 0.25
    for bad in (dict(num_walks=0), dict(walk_length=0), dict(num_walks=-3), dict(restart_prob=1.0), dict(restart_prob=-0.1),
                dict(rank_lo=-1), dict(rank_lo=7, rank_hi=7), dict(rank_lo=9, rank_hi=3), dict(share=1.5), dict(share=-0.01),
                dict(share=float("nan")), dict(num_walks=4097, walk_length=1), dict(num_walks=64, walk_length=65)):
        with pytest.raises(ValueError):
            HardNegatives(**{**dict(rank_lo=5, rank_hi=30), **bad})
    for bad in (1.01, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            hn.share = bad
    assert hn.share == 0.25


def test_c_entries_validate_before_anything_is_enqueued():
    from laplace_amd import _lib
    L = _lib.lib()
    assert L.mi_pinsage_hard_sizeof() == ctypes.sizeof(_lib.PinsageHardNeg) == 32
    fake = 4096

    def direct(W=16, Lw=2, lo=3, hi=10, p=0.5, share=1.0, batch=8):
        hn = _lib.PinsageHardNeg(W, Lw, lo, hi, p, share)
        return L.mi_pinsage_hard_negatives(batch, 100, fake, fake, fake, fake, ctypes.byref(hn), 1, 0, fake, fake, fake, None, None)

    desc = _lib.PinsageBatchDesc(32, 100, fake, fake, fake, fake, 2, 10, 3, 2, 0.5, fake)
    out = _lib.PinsageBatchOut()
    out.seeds = out.pos_u = out.pos_v = out.neg_v = out.counts = fake

    def batch(W=16, Lw=2, lo=3, hi=10, p=0.5, share=1.0):
        hn = _lib.PinsageHardNeg(W, Lw, lo, hi, p, share)
        return L.mi_pinsage_sample_batch_hard(ctypes.byref(desc), ctypes.byref(hn), 1, 0, ctypes.byref(out), fake, 1 << 30, None)

    for call in (direct, batch):
        assert call(W=4097, Lw=1) == _lib.MI_ERR_UNSUPPORTED
        assert call(W=17, Lw=241) == _lib.MI_ERR_UNSUPPORTED            # 4097 slots
        assert call(W=1 << 20, Lw=1 << 20) == _lib.MI_ERR_UNSUPPORTED   # the product does not wrap
        for bad in (dict(W=0), dict(W=-1), dict(Lw=0), dict(p=1.0), dict(p=-0.5), dict(share=1.25), dict(share=-0.5),
                    dict(share=float("nan")), dict(lo=-1), dict(lo=10, hi=10), dict(lo=10, hi=4)):
            assert call(**bad) == _lib.MI_ERR_BAD_ARG, (call.__name__, bad)
    assert L.mi_pinsage_hard_negatives(8, 100, fake, fake, fake, fake, None, 1, 0, fake, fake, fake, None, None) == _lib.MI_ERR_BAD_ARG
    assert direct(batch=-1) == _lib.MI_ERR_BAD_ARG
    assert direct(batch=0) == 0                                         # nothing to do, nothing enqueued
    hn = _lib.PinsageHardNeg(16, 2, 3, 10, 0.5, 1.0)
    assert L.mi_pinsage_hard_negatives(8, 100, fake, fake, fake, fake, ctypes.byref(hn), 1, 0, None, fake, fake, None, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_sample_batch_hard(None, ctypes.byref(hn), 1, 0, ctypes.byref(out), fake, 1 << 30, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_sample_batch_hard(ctypes.byref(desc), ctypes.byref(hn), 1, 0, ctypes.byref(out), fake, 16, None) == _lib.MI_ERR_WORKSPACE
