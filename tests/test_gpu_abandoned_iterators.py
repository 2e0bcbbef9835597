"""GPU: prefetching iterators that are left before their end, and iter_users' order.

DeviceGraphSampler (prefetch on the calling thread and on a thread of its own) and PinSAGESampler.batches keep kernels
queued on side streams.  A consumer that breaks out of an epoch must be able to go on — allocate, overwrite, start the next
epoch — without a device synchronise of its own: closing (or dropping) the iterator orders the consumer's stream after the
queued work, the step counter says how many batches were handed out, and the next epoch is, tensor for tensor, the serial
sampler's epoch from that step.  iter_users checks its ids on the host before anything is uploaded and owns its order from
the moment it is called."""
import gc
from types import SimpleNamespace

import pytest
import torch as t

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, A, B = 210, 90, 16


def _samplers(mode):
    from laplace_amd import synthetic as S
    from laplace_amd.data.device_sampler import DeviceGraphSampler
    spec = S.SyntheticSpec(U, A, 4000, seed=31, deg_min=1, deg_max=A, zipf_s=1.0)
    graph, users, articles = S.generate_hetero(spec, customer_cards=(50, 2, 84), article_cards=(40, 9))
    cfg = SimpleNamespace(k=12, num_neighbors=6, n_hop_neighbors=3, positive_edges_ratio=0.5, negative_edges_ratio=3.0, batch_size=B)
    mk = lambda prefetch: DeviceGraphSampler(cfg, graph, users, articles, batch_size=B, device=DEV, seed=77, prefetch=prefetch)
    return mk(False), mk(mode)


def _tensors(batch):
    """The field list of test_prefetching_epoch_equals_the_serial_epoch (tests/test_gpu_sampler.py)."""
    from laplace_amd.utils.constants import Constants
    out = []
    for nt in (Constants.node_user, Constants.node_item):
        out += [batch[nt].x, batch[nt].n_id]
    for key in ("edge_index", "edge_label_index", "edge_label"):
        out += [batch[Constants.edge_key][key], batch[Constants.rev_edge_key][key]]
    for csr in batch[Constants.edge_key].edge_index._sorted_csr:
        out += [csr.rowptr, csr.col]
    return out


def _same(a, b, what):
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == len(tb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x.shape == y.shape and t.equal(x, y), (what, i)


def _epoch_equals_serial(serial, ahead, what):
    serial.step = ahead.step
    n = 0
    for a, b in zip(serial, ahead):
        _same(a, b, (what, n))
        n += 1
    assert n == len(serial) and serial.step == ahead.step
    return n


def _churn(n_seeds):
    """Memory traffic on the consumer's stream: tensors a few times the size of the epoch's seed order, overwritten (with valid
    ids: zeros) — what would land in a freed seed order if nothing kept it."""
    junk = []
    for k in range(6):
        x = t.empty(max(n_seeds, 1) * (k % 3 + 1), dtype=t.int64, device=DEV)
        x.zero_()
        junk.append(x)
    return junk


@pytest.mark.parametrize("how", ["close", "drop"])
@pytest.mark.parametrize("mode", [True, "thread"])
def test_abandoned_epoch_of_the_device_sampler(mode, how):
    serial, ahead = _samplers(mode)
    it = iter(ahead)
    first = [next(it), next(it)]
    serial_it = iter(serial)
    for i, b in enumerate(first):
        _same(next(serial_it), b, ("before the break", i))
    if how == "close":
        it.close()
    else:
        del it
        gc.collect()
    junk = _churn(U)
    t.cuda.current_stream().synchronize()                 # the consumer's stream only: NOT a device synchronise
    assert ahead._side.query(), "closing the iterator did not order the consumer's stream after the queued chains"
    assert ahead.step == 2                                # the batches handed out, not the batches started
    assert _epoch_equals_serial(serial, ahead, "epoch after the break") == (U + B - 1) // B
    # and once more, broken at another place
    it = iter(ahead)
    for _ in range(5):
        next(it)
    it.close()
    assert ahead.step == 2 + (U + B - 1) // B + 5
    _epoch_equals_serial(serial, ahead, "second epoch after a break")
    del junk, first


@pytest.mark.parametrize("mode", [True, "thread", False])
def test_iter_users_rejects_ids_outside_the_graph_before_any_upload(mode):
    serial, ahead = _samplers(mode)
    _epoch_equals_serial(serial, ahead, "first epoch")
    step = ahead.step
    for bad in (t.tensor([3, U, 5]), t.tensor([3, -1, 5]), t.tensor([U + 1000]), t.tensor([[-7]])):
        with pytest.raises(IndexError):
            ahead.iter_users(bad)
    assert ahead.step == step
    assert list(ahead.iter_users(t.empty(0, dtype=t.int64))) == [] and ahead.step == step
    _epoch_equals_serial(serial, ahead, "epoch after the rejected calls")


@pytest.mark.parametrize("mode", [True, "thread", False])
def test_iter_users_owns_its_order_from_the_call(mode):
    serial, ahead = _samplers(mode)
    g = t.Generator().manual_seed(5)
    u = t.randperm(U, generator=g)[:37]
    step0 = ahead.step
    it = ahead.iter_users(u)
    epoch = iter(ahead)                                    # created after `it` ...
    got = [next(epoch)]                                    # ... and advanced first: it is still the shuffled epoch
    got += list(epoch)
    serial.step = step0
    want = list(serial)
    assert len(got) == len(want) == (U + B - 1) // B
    for i, (a, b) in enumerate(zip(want, got)):
        _same(a, b, ("the epoch", i))
    step1 = ahead.step
    assert step1 == step0 + len(want)
    mine = list(it)                                        # exactly u, in order, from the step the sampler has reached
    assert len(mine) == (37 + B - 1) // B
    for i, b in enumerate(mine):
        chunk = u[i * B:(i + 1) * B]
        assert t.equal(b._seed_users.cpu(), chunk), i
        _same(serial.sample(chunk, step=step1 + i), b, ("iter_users", i))
    assert ahead.step == step1 + len(mine)


def _pin_flat(batch):
    """flat() of test_overlapped_batches_are_the_serial_batches (tests/test_gpu_pinsage_device.py)."""
    return [batch["seeds"], *batch["pos"], *batch["neg"]] + [x for blk in batch["blocks"] for x in (
        blk["src_ids"], blk["edge_src"], blk["edge_dst"], blk["weights"], blk["csr"][0].rowptr, blk["csr"][0].col, blk["csr"][0].val,
        blk["csr"][1].rowptr, blk["csr"][1].col, blk["csr"][1].val)]


@pytest.mark.parametrize("how", ["close", "drop"])
def test_abandoned_batches_of_the_pinsage_sampler(how):
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.sampler import PinSAGESampler
    n_u, n_i = 3000, 900
    ei = S.generate(S.SyntheticSpec(n_u, n_i, 50000, seed=9, deg_min=1, deg_max=60, zipf_s=0.9))
    uu, aa = ei[0].numpy(), ei[1].numpy()
    users, items = AdjList.from_edges(uu, aa, n_u), AdjList.from_edges(aa, uu, n_i)
    mk = lambda: PinSAGESampler(users, items, n_u, n_i, batch_size=48, seed=21)
    a, b = mk(), mk()

    def same(got, what):
        want = a.sample_batch()
        fg, fw = _pin_flat(got), _pin_flat(want)
        assert len(fg) == len(fw)
        for i, (x, y) in enumerate(zip(fg, fw)):
            assert x.shape == y.shape and t.equal(x, y), (what, i)

    it = b.batches(7)
    for i in range(2):
        same(next(it), ("before the break", i))
    if how == "close":
        it.close()
    else:
        del it
        gc.collect()
    junk = _churn(48 * 64)
    assert b.step == a.step == 2                          # the batches handed out; two more chains were in flight
    n = 0
    for got in b.batches(5):                              # the next call continues the sequence from there
        same(got, ("after the break", n))
        n += 1
    assert n == 5 and b.step == a.step == 7
    t.cuda.synchronize()
    assert bool((b._pos32 == -1).all()) and all(bool((p == -1).all()) for p in b._lane_pos)   # every scratch handed back clean
    del junk
