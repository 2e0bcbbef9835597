"""What the one-C-call executors' host sides share (ranker_native.NativeRankerStep / NativeRankerForward,
pinsage.native.NativePinSAGEStep, pinsage.model.ItemProjector): torch.optim.Adam's state as the executors read and write it, the
flat gradient buffer, the workspace growth rule (grown_workspace), the test for a stale raw-pointer descriptor, and the collective
accept / decline of a data-parallel step.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence

import torch as t
from torch import Tensor


# ---- torch.optim.Adam, as the executors take it ------------------------------------------------------------------------------
def adam_unsupported_reason(optimizer) -> Optional[str]:
    if type(optimizer) is not t.optim.Adam or len(optimizer.param_groups) != 1:
        return "optimizer other than a single-group torch.optim.Adam"
    g = optimizer.param_groups[0]
    if g.get("amsgrad") or g.get("weight_decay", 0) or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
        return "Adam options (amsgrad / weight_decay / maximize / capturable)"
    return None


def ensure_adam_state(optimizer, group: dict, p: Tensor) -> dict:
    """optimizer.state[p], created the way torch.optim.Adam creates it on its first step."""
    st = optimizer.state[p]
    if len(st) == 0:
        on_device = bool(group.get("fused") or group.get("capturable"))
        st["step"] = t.zeros((), dtype=t.float32, device=p.device) if on_device else t.tensor(0.0, dtype=t.float32)
        st["exp_avg"] = t.zeros_like(p, memory_format=t.preserve_format)
        st["exp_avg_sq"] = t.zeros_like(p, memory_format=t.preserve_format)
    return st


def bind_param(q, p: Tensor, grad: Tensor, state: dict) -> None:
    """One _lib.RankerParam slot `q`: parameter, gradient, the two moments, the element count."""
    q.p, q.g, q.m, q.v, q.n = p.data_ptr(), grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), p.numel()


def bump_adam_steps(steps: Sequence[Tensor]) -> None:
    if steps and steps[0].is_cuda:      # fused=True keeps its step counts on the device: one foreach launch
        t._foreach_add_(list(steps), 1)
    else:
        for s in steps:                 # the default Adam's host scalars
            s += 1


def flat_grad_views(params: Sequence[Tensor], flat: Optional[Tensor], *, keep_values: bool) -> Optional[Tensor]:
    """One float32 buffer whose 16-byte aligned pieces are the params' `.grad`s (a data-parallel caller exchanges it in one
    collective).  `flat` is returned as it is when every p.grad already is its view; otherwise a new zero-filled buffer, into
    which keep_values=True copies every existing gradient of its parameter's shape."""
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4
    if not params or (flat is not None and flat.numel() == total and all(
            p.grad is not None and p.grad.data_ptr() == flat.data_ptr() + 4 * o for p, o in zip(params, offs))):
        return flat
    flat = t.zeros(total, dtype=t.float32, device=params[0].device)
    for p, o in zip(params, offs):
        view = flat[o: o + p.numel()].view(p.shape)
        if keep_values and p.grad is not None and p.grad.shape == p.shape:
            view.copy_(p.grad)
        p.grad = view
    return flat


# ---- the executors' workspace -------------------------------------------------------------------------------------------------
def grown_workspace(current: Optional[Tensor], need: int, device) -> Tensor:
    """`current` when it holds `need` bytes; else a new one of `need` + 25 % + 1 MiB, so that the next, slightly larger batch
    does not allocate again.  current=None always allocates."""
    if current is not None and current.numel() >= need:
        return current
    return t.empty(int(need * 1.25) + (1 << 20), dtype=t.uint8, device=device)


# ---- stale descriptors ----------------------------------------------------------------------------------------------------------
class PointerSnapshot:
    """A descriptor holds raw pointers; this holds how to find the tensors it was built from and where they were then.
    `getters`: zero-argument callables that return a tensor, None, or a tuple / list of those.  `optimizer`: every parameter of
    its (one) group with its gradient and two moments as well.  current() is False once any of them gives another address, a
    tensor where there was none or the reverse (zero_grad(set_to_none=True)), or raises (a missing optimizer state), or once the
    optimizer's parameter list is no longer the same objects in the same order.
    Addresses are kept as Python ints: reading them back out of a ctypes descriptor (four fields x ~25 tensors) was 30 us of the
    ranker's host-bound 0.47 ms iteration."""

    def __init__(self, getters: Iterable[Callable] = (), optimizer=None):
        self._getters, self._optimizer = list(getters), optimizer
        self._ptrs = self._pointers()
        self._rows = []
        if optimizer is not None:
            state = optimizer.state
            self._rows = [(p, p.data_ptr(), p.grad.data_ptr(), state[p]["exp_avg"].data_ptr(), state[p]["exp_avg_sq"].data_ptr())
                          for p in optimizer.param_groups[0]["params"]]

    def _pointers(self) -> List[Optional[int]]:
        out = []
        for get in self._getters:
            x = get()
            for y in (x if type(x) in (tuple, list) else (x,)):
                out.append(None if y is None else y.data_ptr())
        return out

    def current(self) -> bool:
        try:
            if self._optimizer is not None:
                params, state = self._optimizer.param_groups[0]["params"], self._optimizer.state
                if len(params) != len(self._rows):
                    return False
                for p, (q, pp, gp, mp, vp) in zip(params, self._rows):
                    g, st = p.grad, state.get(p)
                    if (p is not q or g is None or not st or p.data_ptr() != pp or g.data_ptr() != gp
                            or st["exp_avg"].data_ptr() != mp or st["exp_avg_sq"].data_ptr() != vp):
                        return False
            return self._pointers() == self._ptrs
        except Exception:
            return False


# ---- the collective decision ------------------------------------------------------------------------------------------------------
def all_ranks_take_it(mine: bool, device, group) -> bool:
    """Data-parallel only: the decline is COLLECTIVE.  A rank whose batch lies outside the executor's shapes must not leave its
    peers alone in the gradient exchange (they would wait for the collective's timeout, or reduce against the fallback path's
    differently sized buffer): one all-reduce(MIN) of a 1-int flag BEFORE anything is enqueued, and every rank takes the same
    branch."""
    import torch.distributed as dist
    flag = t.tensor([1 if mine else 0], dtype=t.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    return bool(int(flag.item()))


PEER_DECLINED = "a peer rank declined its batch (collective decision: every rank takes the fallback)"


def collective_prepare(world: int, vote: Callable[[bool], bool], prepare: Callable[[], object]):
    """(prepare(), whether to go on).  prepare() returns None to decline, and enqueues nothing.  With world > 1 the ranks vote:
    all go on or none does — and a rank whose prepare() raises answers the vote with "no" before it fails, because its peers are
    already on their way into it."""
    try:
        prep = prepare()
    except BaseException:
        if world > 1:
            vote(False)
        raise
    if world > 1:
        return prep, vote(prep is not None)
    return prep, prep is not None
