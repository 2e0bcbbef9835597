"""GPU: every code path the top-K dispatcher can pick (csrc/topk.hip: M, M1, G, D, P — include/laplace_hip.h, mi_topk_path),
on the case table of tests/topk_cases.py.  For each case: the dispatcher's own decision function says the call takes the path
the case was written for (with the prefilter on: a P case must report P on the device), the ids of EVERY query row equal the
oracle's exact selection over its fma-chain scores (oracle/spmm_ref.c), and the returned scores are the oracle's bits at every
position that is not a -1 pad.  Nothing here has a tolerance.  Strided, offset and aliased layouts give the oracle contiguous
copies of the same values.  tests/test_topk_paths_cpu.py checks the same table's paths and coverage without a GPU.

The GEMM's row gather (scores = U[uid] @ I^T, `a_rows` of csrc/gemm.hpp) has no entry point of its own: mi_gemm_f32 passes no
gather.  It is reached through the materialised top-K instead, asked for ALL items of a block with their scores
(test_gemm_row_gather_scores_every_item_bitwise)."""
import os
import sys

import pytest
import torch as t

from oracle import lightgcn_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _csr(b, n_q, n_items):
    from laplace_amd import ops
    if b["rowptr"] is None:
        return None
    return ops.DeviceCSR(n_q, n_items, b["rowptr"].to(DEV), b["col"].to(DEV))


def _check_layout(c, ue, ie):
    """The tensors really have the alignment and leading dimensions the CPU test asked mi_topk_path about."""
    from laplace_amd import ops
    up, ldu, ip, ldi = T.layout_of(c, 0, 0)
    assert ue.untyped_storage().data_ptr() % 256 == 0 and ie.untyped_storage().data_ptr() % 256 == 0
    assert ue.data_ptr() % 16 == up % 16 and ie.data_ptr() % 16 == ip % 16
    assert ops._rows_ok(ue, "ue") == ldu and ops._rows_ok(ie, "ie") == ldi
    if c.layout in ("halves", "same"):
        assert ie.data_ptr() - ue.data_ptr() == ip - up


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_case_runs_its_declared_path_and_equals_the_oracle(case, monkeypatch):
    from laplace_amd import ops
    c = case
    monkeypatch.setenv("LAPLACE_TOPK_PREFILTER", "1")
    b = T.build(c, DEV)
    ue, ie, uid = b["ue"], b["ie"], b["uid"]
    _check_layout(c, ue, ie)
    # 1. the path: asked of the function the dispatcher calls, on the pointers the call gets
    got_path = ops.topk_path(ue, ie, c.k)
    assert got_path == c.path, (T.PATH_NAMES.get(got_path, got_path), T.PATH_NAMES[c.path])
    scores = R.scores_fma(b["ue_ref"][uid], b["ie_ref"])
    if b["need_scores"]:
        T.finish_excl(c, b, scores)
    ex = _csr(b, c.n_q, c.n_items)
    excl = b["excl"] if b["excl"] is not None else [t.empty(0, dtype=t.int64)] * c.n_q
    want = R.topk_excl_exact(scores, excl, c.k)
    valid = want >= 0
    want_sc = scores.gather(1, want.clamp(min=0))
    if c.excl == "all":
        assert not bool(valid[0].any())                    # the row that excludes everything is all pads
    if c.excl == "leave_k-1":
        assert int(valid[0].sum()) == c.k - 1
    uid_d = uid.to(DEV)

    def call():
        if c.want_scores:
            return ops.topk_excl(uid_d, ue, ie, c.k, ex, want_scores=True)
        return ops.topk_excl(uid_d, ue, ie, c.k, ex), None

    # 2. ids of every query row, 3. scores bit for bit wherever there is an item
    ids, sc = call()
    assert ids.shape == (c.n_q, c.k)
    bad = (ids.cpu() != want).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{bad.numel()} of {c.n_q} rows differ, first: row {int(bad[0])}"
    if c.want_scores:
        assert t.equal(sc.cpu()[valid], want_sc[valid])
    # the tables were not written to
    assert t.equal(ue.cpu(), b["ue_ref"]) and t.equal(ie.cpu(), b["ie_ref"])
    # P: the same call with the prefilter off runs D and returns the same bits
    if c.path == T.P:
        monkeypatch.setenv("LAPLACE_TOPK_PREFILTER", "0")
        assert ops.topk_path(ue, ie, c.k) == T.D
        ids_f, sc_f = call()
        assert t.equal(ids_f, ids)
        if c.want_scores:
            assert t.equal(sc_f.cpu()[valid], sc.cpu()[valid])
        monkeypatch.setenv("LAPLACE_TOPK_PREFILTER", "1")
    # the same call cut into chunks (the last one smaller), over two streams and two workspaces, then over one
    if c.chunk:
        monkeypatch.setattr(ops, "TOPK_WS_BYTES", 4 * c.n_items * c.chunk)
        monkeypatch.setattr(ops, "TOPK_CHUNK_QUANTUM", c.chunk)
        for streams in (2, 1):
            monkeypatch.setattr(ops, "TOPK_STREAMS", streams)
            ids_c, sc_c = call()
            assert t.equal(ids_c, ids), streams
            if c.want_scores:
                assert t.equal(sc_c, sc), streams


@pytest.mark.parametrize("layout", ["contig", "ld+1"])
@pytest.mark.parametrize("n_q,n_items,d", [(1, 1, 1), (65, 130, 50), (300, 1000, 33), (257, 4096, 200)])
def test_gemm_row_gather_scores_every_item_bitwise(n_q, n_items, d, layout):
    """scores = U[uid] @ I^T through the GEMM's row gather, every element against the oracle's fma chain.  The route: the
    materialised top-K (path M) asked for k = all items of a block of <= 1 024 with their scores, everything outside the block
    excluded — the union of the blocks is the whole score matrix.  Contiguous d = 200 takes gemm_fast_kernel<true, true>
    (float4-addressable rows); d = 1, 33, 50 and every ld = d + 1 layout take gemm_f32_kernel with the gather."""
    from laplace_amd import ops
    g = t.Generator().manual_seed(n_q * 7 + n_items + d)
    U = n_q + 9
    ue_ref, ie_ref = t.randn(U, d, generator=g), t.randn(n_items, d, generator=g)
    uid = t.randint(0, U, (n_q,), generator=g)                       # unsorted, with repeats
    ld = d + 1 if layout == "ld+1" else d

    def dev(x):
        buf = t.full((x.shape[0], ld), float("nan"), device=DEV)
        buf[:, :d] = x.to(DEV)
        return buf[:, :d]
    ue, ie = dev(ue_ref), dev(ie_ref)
    want = R.scores_fma(ue_ref[uid], ie_ref)
    got = t.full((n_q, n_items), float("nan"))
    block = 1024
    for b0 in range(0, n_items, block):
        b1 = min(n_items, b0 + block)
        k = b1 - b0
        assert ops.topk_path(ue, ie, k) == T.M
        outside = t.cat([t.arange(0, b0), t.arange(b1, n_items)])
        ex = None
        if outside.numel():
            rowptr = (t.arange(n_q + 1) * outside.numel()).to(t.int32)
            ex = ops.DeviceCSR(n_q, n_items, rowptr.to(DEV), outside.repeat(n_q).to(t.int32).to(DEV))
        ids, sc = ops.topk_excl(uid.to(DEV), ue, ie, k, ex, want_scores=True)
        ids, sc = ids.cpu(), sc.cpu()
        assert t.equal(ids, R.topk_excl_exact(want, [outside] * n_q, k))
        assert t.equal(ids.sort(1).values, t.arange(b0, b1).repeat(n_q, 1))    # every item of the block, once
        got.scatter_(1, ids, sc)
    assert t.equal(got, want)
