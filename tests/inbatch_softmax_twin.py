"""The in-batch sampled softmax of include/laplace_hip.h ("In-batch sampled softmax") in torch, under autograd, on the CPU:
the yardstick of tests/test_inbatch_softmax_cpu.py and tests/test_gpu_inbatch_softmax.py, and the shared kernel cases."""
import functools

import torch as t


def twin_loss(f, e, n_users, users, pos, group, lam, logq):
    """The loss on tables f (final) and e (layer 0) of any dtype; logq [n_items] or None.  One dense score block per group."""
    B = users.numel()
    main = f.new_zeros(())
    for g0 in range(0, B, group):
        u, p = users[g0:g0 + group], pos[g0:g0 + group]
        logit = f[u] @ f[n_users + p].T                      # [slot b, candidate j]
        if logq is not None:
            logit = logit - logq.to(f.dtype)[p][None, :]
        n = u.numel()
        own = t.eye(n, dtype=t.bool)
        masked = ((p[None, :] == p[:, None]) | (u[None, :] == u[:, None])) & ~own
        lse = t.logsumexp(logit.masked_fill(masked, float("-inf")), dim=1)
        main = main + (lse - logit.diagonal()).sum()
    return main / B + lam * (e[users].pow(2).sum() + e[n_users + pos].pow(2).sum())


def twin(final, e0, n_users, users, pos, group, lam, logq, dtype):
    """(loss, dL/dfinal, dL/de0) in `dtype` by autograd over the rule."""
    f = final.detach().to(dtype).clone().requires_grad_(True)   # a copy also when dtype is the input's: the inputs stay as they are
    e = e0.detach().to(dtype).clone().requires_grad_(True)
    loss = twin_loss(f, e, n_users, users, pos, group, lam, logq)
    loss.backward()
    return loss.detach(), f.grad, e.grad


# (B, G, d, users, items)
SHAPES = ((33, 32, 8, 40, 50),        # a one-slot tail group
          (17, 32, 16, 17, 17),       # one partial group; every user and every item once
          (64, 32, 32, 40, 50),       # two full groups
          (100, 32, 64, 5, 6),        # almost everything masked; the rows of user 0 and item 0 cross 64-reference chunks
          (200, 64, 100, 300, 200),
          (256, 128, 128, 300, 200),
          (64, 64, 256, 40, 50),      # the widest rows
          (2048, 1024, 128, 3000, 2000))   # many tiles per group in both sweeps


@functools.lru_cache(maxsize=None)
def cases():
    """The kernel cases with their seeded inputs, built once and left unchanged:
    dicts of B, G, d, U, I, final [U + I, d], e0 [U + I, d], logq [I], users [B], pos [B]."""
    out = []
    for i, (B, G, d, U, I) in enumerate(SHAPES):
        g = t.Generator().manual_seed(1000 + i)
        final = 0.3 * t.randn(U + I, d, generator=g)
        e0 = t.randn(U + I, d, generator=g)
        logq = t.log(0.1 * t.rand(I, generator=g) + 1e-4)
        if (U, I) == (B, B):          # distinct ids: no mask
            users, pos = t.randperm(U, generator=g), t.randperm(I, generator=g)
        elif U <= 8:                  # a skewed handful of ids: user 0 and item 0 take most slots
            pu = t.tensor([0.7] + [0.3 / (U - 1)] * (U - 1))
            pi = t.tensor([0.7] + [0.3 / (I - 1)] * (I - 1))
            users = t.multinomial(pu, B, replacement=True, generator=g)
            pos = t.multinomial(pi, B, replacement=True, generator=g)
        else:
            users, pos = t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g)
        out.append(dict(B=B, G=G, d=d, U=U, I=I, final=final, e0=e0, logq=logq, users=users, pos=pos))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(i, lam, with_logq):
    """The float64 twin of case i: computed once, shared by the tests."""
    c = cases()[i]
    return twin(c["final"], c["e0"], c["U"], c["users"], c["pos"], c["G"], lam, c["logq"] if with_logq else None, t.float64)
