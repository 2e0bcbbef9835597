"""The full-catalogue softmax of include/laplace_hip.h ("Full-catalogue softmax") in torch, under autograd, on the CPU: the
yardstick of tests/test_full_softmax_cpu.py and tests/test_gpu_full_softmax.py, and the shared kernel cases.

What the cases put through the kernel's decomposition (csrc/fullsoftmax.hip, split_catalogue: enough item chunks of whole
32-item tiles for 8 192 wavefronts, at most 32, at least one tile each; chunks = ceil(tiles / ceil(tiles / wanted))):
case 7, (2048, 128, 3000, 2000), has 64 user blocks and 63 item tiles, so 32 chunks are wanted, a chunk is 2 tiles, and the
32nd chunk is partial: one tile, of 16 items — many chunks with a partial last one through the (max, sum) merge and the
partial-row sum.  Case 6, (256, 128, 300, 4133), has 8 user blocks against 26 chunks of 5 tiles, the last tile with 5 items;
case 4 has 7 one-tile chunks.  Case 0, (33, 8, 40, 50), has two owned user blocks, the last with one slot, and two owned
item blocks, the last with 18 items.  Cases 1, 3 and 8 are one chunk: the statistics merge of one pair and no partial-row sum.
No further case is needed."""
import functools

import torch as t


def twin_loss(f, e, n_users, users, pos, lam):
    """The loss on tables f (final) and e (layer 0) of any dtype: one dense [B, I] logit block."""
    B = users.numel()
    logit = f[users] @ f[n_users:].T                         # [slot b, item i]
    main = (t.logsumexp(logit, dim=1) - logit[t.arange(B), pos]).sum()
    return main / B + lam * (e[users].pow(2).sum() + e[n_users + pos].pow(2).sum())


def twin(final, e0, n_users, users, pos, lam, dtype):
    """(loss, dL/dfinal, dL/de0) in `dtype` by autograd over the rule."""
    f = final.detach().to(dtype).clone().requires_grad_(True)   # a copy also when dtype is the input's: the inputs stay as they are
    e = e0.detach().to(dtype).clone().requires_grad_(True)
    loss = twin_loss(f, e, n_users, users, pos, lam)
    loss.backward()
    return loss.detach(), f.grad, e.grad


# (B, d, users, items)
SHAPES = ((33, 8, 40, 50),          # partial user tile, partial item tile
          (17, 16, 17, 17),         # less than one tile a side
          (64, 32, 40, 64),         # whole tiles exactly
          (100, 64, 5, 6),          # fewer items than a tile, every id repeats many times (cross 64-reference chunks)
          (200, 100, 300, 200),     # d not a multiple of 32
          (64, 256, 40, 50),        # the widest rows
          (256, 128, 300, 4133),    # many item tiles, a ragged tail: 8 chunks, the last partial
          (2048, 128, 3000, 2000),  # many tiles both ways
          (96, 4, 7, 1))            # one item: main term exactly 0, gradients exactly 0


@functools.lru_cache(maxsize=None)
def cases():
    """The kernel cases with their seeded inputs, built once and left unchanged:
    dicts of B, d, U, I, final [U + I, d], e0 [U + I, d], users [B], pos [B]."""
    out = []
    for i, (B, d, U, I) in enumerate(SHAPES):
        g = t.Generator().manual_seed(2000 + i)
        final = 0.3 * t.randn(U + I, d, generator=g)
        e0 = t.randn(U + I, d, generator=g)
        users, pos = t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g)
        out.append(dict(B=B, d=d, U=U, I=I, final=final, e0=e0, users=users, pos=pos))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(i, lam):
    """The float64 twin of case i: computed once, shared by the tests."""
    c = cases()[i]
    return twin(c["final"], c["e0"], c["U"], c["users"], c["pos"], lam, t.float64)
