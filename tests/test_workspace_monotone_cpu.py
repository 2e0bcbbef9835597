"""CPU: is the native ranker executor's workspace need monotone in the batch dims?  (ranker_native.NativeRankerStep skips the
counting pass for a batch no larger in any of (customers, articles, edges, label edges) than one it has sized.)

The counting pass (mi_ranker_step_workspace_bytes) is host-only — tests/asan_driver.py drives it with made-up addresses —
so both facts are pinned here without a GPU:
  * the suite's model (first-layer widths 64 / 56): no violation over a fixed random set of ordered dim pairs;
  * a customer input width of 512: the COUNTED need is not monotone.  The GEMMs' split-K partials depend on the output's
    tile count (mi_gemm_splits: an output of <= 8 tiles splits K from 512 on, a ninth tile stops it), so a batch with one
    more article and four times the edges is counted at LESS than the smaller one (measured: 212 069 120 B against
    211 984 640 B).  The count is an upper bound of what the validation and launch passes take (they group GEMMs the
    count sizes one by one): for this pair the smaller batch still FITS the larger one's count (it uses 211 540 736 B),
    which is pinned too.  NativeRankerStep therefore treats the skipped count as a bet and recovers from MI_ERR_WORKSPACE
    (tests/test_gpu_second_call.py).  If a change to the GEMM's split rule removes the violation this test fails and says
    so: the pair below, and ranker_native's comment, are then out of date."""
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asan_driver import L, _lib, ranker_case  # noqa: E402

SMALL, BIG = (20000, 256, 1024, 300), (20000, 257, 4096, 300)      # (n_c, n_a, nnz, n_label): BIG >= SMALL in every count


def _case(dims, width=64):
    """ranker_case at these batch dims; width > 64 widens the customers' first embedding column (and with it the first
    layer's customer-side weights) to that input width."""
    n_c, n_a, nnz, n_label = dims
    d, b, f = ranker_case(n_c=n_c, n_a=n_a, nnz=nnz, n_label=n_label)
    if width != 64:
        assert width > 64 and width % 4 == 0
        col = int(d.dims[0][0]) + width - 64
        d.dims[0][0] = col
        d.tables[0][0] = f(4 * col * int(d.table_rows[0][0]))
        assert sum(int(d.dims[0][c]) for c in range(int(d.n_cols[0]))) == width
        # the two weights that take the customers' input: lin_l of customer -> article, lin_r of article -> customer
        for cv, side, pi in ((d.conv[0][0], "l", 0), (d.conv[0][1], "r", 5)):
            n = int(cv.c_out) * width
            q = d.params[pi]
            assert int(q.p) == int(getattr(cv, "w_" + side))          # the optimizer entry of that very weight
            q.p, q.g, q.m, q.v, q.n = f(4 * n), f(4 * n), f(4 * n), f(4 * n), n
            setattr(cv, "w_" + side, q.p)
            setattr(cv, "gw_" + side, q.g)
            if side == "l":
                cv.c_src = width
            else:
                cv.c_dst = width
    return d, b, f


def _need(dims, width=64):
    d, b, f = _case(dims, width)
    need = int(L.mi_ranker_step_workspace_bytes(ctypes.byref(d), ctypes.byref(b)))
    assert need > 0, (dims, width)                                     # 0 = a descriptor the executor does not take
    rc = int(L.mi_ranker_step_check(ctypes.byref(d), ctypes.byref(b), f(need), need))
    assert rc == 0, (dims, width, rc)                                  # the validation pass accepts it at exactly that size
    return need


def _pairs(n, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        small = (rnd.randint(1, 40000), rnd.randint(1, 12000), rnd.randint(0, 60000), rnd.randint(1, 4000))
        grow = [rnd.choice((0, 0, 1, rnd.randint(1, 64), rnd.randint(1, 20000))) for _ in range(4)]
        out.append((small, tuple(s + g for s, g in zip(small, grow))))
    return out


def test_width_64_is_monotone_over_a_fixed_random_set_of_dim_pairs():
    worst = None
    for small, big in _pairs(500, seed=20240):
        ns, nb = _need(small), _need(big)
        if ns > nb and (worst is None or ns - nb > worst[0]):
            worst = (ns - nb, small, big, ns, nb)
    assert worst is None, f"a smaller batch needs more workspace at width 64: {worst}"


def test_width_512_count_is_not_monotone():
    ns, nb = _need(SMALL, 512), _need(BIG, 512)
    print(f"width 512: need{SMALL} = {ns} B, need{BIG} = {nb} B")
    assert ns > nb, ("the violating pair no longer violates: has mi_gemm_splits changed?  Then correct this test and the "
                     "comment in ranker_native.NativeRankerStep._prepare", ns, nb)
    # what the validation pass (the launch pass's twin) takes is below the count: in exactly the larger batch's counted bytes
    # the smaller batch is accepted; cut below its own use it is declined with the code NativeRankerStep recovers from
    d, b, f = _case(SMALL, 512)
    ws = f(ns)
    assert int(L.mi_ranker_step_check(ctypes.byref(d), ctypes.byref(b), ws, nb)) == 0
    assert int(L.mi_ranker_step_check(ctypes.byref(d), ctypes.byref(b), ws, nb // 2)) == _lib.MI_ERR_WORKSPACE
    # the same pair at the suite's width is monotone
    assert _need(SMALL) <= _need(BIG)
