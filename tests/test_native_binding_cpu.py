"""CPU: native_binding — what the one-C-call executors' host sides share.  Adam's state as torch.optim.Adam itself leaves it, the
stale-descriptor test (PointerSnapshot), the flat gradient buffer, and the vote of a rank whose prepare raises."""
import pytest
import torch as t

from laplace_amd import native_binding as NB


def test_adam_state_is_what_torch_leaves_after_a_zero_gradient_step():
    t.manual_seed(0)
    p = t.nn.Parameter(t.randn(3, 5))
    twin = t.nn.Parameter(p.detach().clone())
    opt, opt_twin = t.optim.Adam([p], lr=1e-2), t.optim.Adam([twin], lr=1e-2)
    twin.grad = t.zeros_like(twin)
    opt_twin.step()
    st = NB.ensure_adam_state(opt, opt.param_groups[0], p)
    assert st is opt.state[p] and NB.ensure_adam_state(opt, opt.param_groups[0], p) is st
    NB.bump_adam_steps([st["step"]])
    want = opt_twin.state[twin]
    assert list(st.keys()) == list(want.keys())
    for k in want:
        assert (st[k].dtype, st[k].device, st[k].shape) == (want[k].dtype, want[k].device, want[k].shape), k
        assert t.equal(st[k], want[k]), k
    assert st["step"].dtype == t.float32 and st["step"].dim() == 0 and float(st["step"]) == 1.0
    assert t.equal(p, twin)                                             # a zero gradient moves nothing


def test_adam_unsupported_reason():
    p = t.nn.Parameter(t.zeros(2))
    assert NB.adam_unsupported_reason(t.optim.Adam([p])) is None
    assert NB.adam_unsupported_reason(t.optim.SGD([p], lr=0.1)) is not None
    assert NB.adam_unsupported_reason(t.optim.AdamW([p])) is not None
    assert NB.adam_unsupported_reason(t.optim.Adam([{"params": [p]}, {"params": [t.nn.Parameter(t.zeros(1))]}])) is not None
    for opts in (dict(amsgrad=True), dict(weight_decay=0.1), dict(maximize=True)):
        assert "Adam options" in NB.adam_unsupported_reason(t.optim.Adam([p], **opts)), opts


def _adam_with_state(n=3):
    params = [t.nn.Parameter(t.randn(4, 2)) for _ in range(n)]
    opt = t.optim.Adam(params)
    for p in params:
        p.grad = t.zeros_like(p)
        NB.ensure_adam_state(opt, opt.param_groups[0], p)
    return params, opt


def test_pointer_snapshot():
    params, opt = _adam_with_state()
    box = {"buffer": t.zeros(3), "absent": None}
    take = lambda: NB.PointerSnapshot([lambda: box["buffer"], lambda: (box["absent"], box["buffer"]), lambda: [box["buffer"]]], optimizer=opt)
    snap = take()
    assert snap.current() and snap.current()
    box["buffer"] = box["buffer"].clone()                               # one tensor replaced by a clone
    assert not snap.current()
    snap = take()
    assert snap.current()
    box["absent"] = t.zeros(1)                                          # a tensor where there was none
    assert not snap.current()
    snap = take()
    params[1].grad = None                                               # zero_grad(set_to_none=True)
    assert not snap.current()
    params[1].grad = t.zeros_like(params[1])
    assert not snap.current()                                           # another buffer came back
    snap = take()
    assert snap.current()
    opt.state[params[2]]["exp_avg_sq"] = opt.state[params[2]]["exp_avg_sq"].clone()     # an optimizer-state entry replaced
    assert not snap.current()
    snap = take()
    del opt.state[params[0]]                                            # ... or missing: the getter raises
    assert not snap.current()
    NB.ensure_adam_state(opt, opt.param_groups[0], params[0])
    snap = take()
    assert snap.current()
    extra = t.nn.Parameter(t.zeros(2))
    opt.param_groups[0]["params"].append(extra)                         # the parameter list grows by one
    assert not snap.current()
    extra.grad = t.zeros_like(extra)
    NB.ensure_adam_state(opt, opt.param_groups[0], extra)
    snap = take()
    assert snap.current()
    twin = t.nn.Parameter(extra.detach())                               # another object over the same storage, same everything else
    twin.grad, opt.state[twin] = extra.grad, opt.state[extra]
    opt.param_groups[0]["params"][-1] = twin
    assert twin.data_ptr() == extra.data_ptr() and not snap.current()
    assert take().current()


@pytest.mark.parametrize("keep_values", [True, False])
def test_flat_grad_views(keep_values):
    params = [t.nn.Parameter(t.randn(n)) for n in (1, 5, 12)] + [t.nn.Parameter(t.randn(3, 3))]
    params[1].grad = t.full((5,), 2.0)
    flat = NB.flat_grad_views(params, None, keep_values=keep_values)
    assert flat.dtype == t.float32 and flat.numel() == 4 + 8 + 12 + 12
    for p, off in zip(params, (0, 4, 12, 24)):
        assert p.grad.shape == p.shape and p.grad.data_ptr() == flat.data_ptr() + 4 * off and off % 4 == 0
    assert float(flat.sum()) == (10.0 if keep_values else 0.0)
    assert t.equal(params[1].grad, t.full((5,), 2.0 if keep_values else 0.0))
    params[0].grad.fill_(3.0)
    again = NB.flat_grad_views(params, flat, keep_values=keep_values)  # every p.grad is its view already: reused, untouched
    assert again is flat and again.data_ptr() == flat.data_ptr() and float(params[0].grad[0]) == 3.0
    params[3].grad = None                                               # one view dropped: a new buffer
    fresh = NB.flat_grad_views(params, flat, keep_values=keep_values)
    assert fresh is not flat and params[3].grad.data_ptr() == fresh.data_ptr() + 4 * 24
    assert float(params[0].grad[0]) == (3.0 if keep_values else 0.0)
    assert NB.flat_grad_views([], None, keep_values=keep_values) is None


def test_a_raising_prepare_votes_no_first():
    votes = []
    vote = lambda mine: votes.append(mine) or mine

    def boom():
        raise RuntimeError("descriptor build failed")
    with pytest.raises(RuntimeError, match="descriptor build failed"):
        NB.collective_prepare(2, vote, boom)
    assert votes == [False]
    with pytest.raises(RuntimeError, match="descriptor build failed"):
        NB.collective_prepare(1, vote, boom)
    assert votes == [False]                                             # a single process casts no vote
    assert NB.collective_prepare(1, vote, lambda: "prep") == ("prep", True)
    assert NB.collective_prepare(1, vote, lambda: None) == (None, False)
    assert votes == [False]
    assert NB.collective_prepare(2, vote, lambda: "prep") == ("prep", True) and votes == [False, True]
    assert NB.collective_prepare(2, vote, lambda: None) == (None, False) and votes == [False, True, False]
    assert NB.collective_prepare(2, lambda mine: False, lambda: "prep") == ("prep", False)     # a peer declined
