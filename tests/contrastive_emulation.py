"""The noise-view contrastive term of include/laplace_hip.h ("Noise-view contrastive term") restated on the CPU: the noise in
numpy on oracle/philox.py, the contrast and the perturbed LightGCN forward in torch (any dtype, float64 for the yardstick).
Shared by tests/test_contrastive_cpu.py and tests/test_gpu_contrastive.py."""
import functools

import numpy as np
import torch as t

from oracle import lightgcn_ref as R
from oracle.philox import philox4x32

TAG = 0x58434C31
GOLDEN = 0x9E3779B97F4A7C15
FLOOR = 1e-12


def key(seed, step):
    s = (int(seed) + GOLDEN * int(step)) & (2 ** 64 - 1)
    return s & 0xFFFFFFFF, s >> 32


def uniforms(ids, d, layer, seed, step):
    """u [len(ids), d] float32, exact: column c is word c % 4 of the block at counter (id, c / 4, layer, TAG)."""
    ids = np.asarray(ids, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k0, k1 = key(seed, step)
    blocks = np.arange(d // 4, dtype=np.uint64)
    w = philox4x32(ids[:, None], blocks[None, :], layer, TAG, k0, k1)            # 4 x [n, d / 4]
    w = np.stack(w, axis=-1).reshape(len(ids), d)                                 # word j of block e -> column 4 e + j
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u


def noise(ids, d, layer, seed, step):
    """n [len(ids), d] float64: the rows of u divided by their norms (float64 sums)."""
    u = uniforms(ids, d, layer, seed, step).astype(np.float64)
    return u / np.maximum(np.sqrt((u * u).sum(axis=1, keepdims=True)), FLOOR)


def perturb(y, eps, layer, seed, step, row_ids=None):
    """X = Y + eps * sign(Y) * n in float64, Y a numpy array [n_rows, d]; row_ids None: the row's own index."""
    y = np.asarray(y, dtype=np.float64)
    ids = np.arange(y.shape[0]) if row_ids is None else np.asarray(row_ids)
    return y + eps * np.sign(y) * noise(ids, y.shape[1], layer, seed, step)


def perturb_bound(y, eps):
    """|X_kernel - X_mirror| per element.  u is exact; the kernel's norm is a sum of d fp32 products (relative error at most
    (d + 1) 2^-24 on the sum, half of it after the root, plus the root's and the division's roundings), the factor
    eps / norm and its product with sign(y) u round once each, and the final fma rounds X once (|X| <= |Y| + eps):
    eps * (d + 8) * 2^-24 + 2^-23 * |Y| covers them."""
    d = y.shape[1]
    return eps * (d + 8) * 2.0 ** -24 + 2.0 ** -23 * np.abs(np.asarray(y, dtype=np.float64))


# ------------------------------------------------------------------------------------ the contrast
def _normalise(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(FLOOR)


def contrast_loss(a, b, ids, tau, group):
    """(1/B) sum_b [ logsumexp_j l[b, j] - l[b, b] ], l = <p_b, q_j> / tau over b's group, other slots of b's id masked."""
    B = ids.numel()
    p, q = _normalise(a[ids]), _normalise(b[ids])
    total = a.new_zeros(())
    for g0 in range(0, B, group):
        i = ids[g0:g0 + group]
        logit = p[g0:g0 + group] @ q[g0:g0 + group].T / tau
        own = t.eye(i.numel(), dtype=t.bool)
        masked = (i[None, :] == i[:, None]) & ~own
        lse = t.logsumexp(logit.masked_fill(masked, float("-inf")), dim=1)
        total = total + (lse - logit.diagonal()).sum()
    return total / B


def contrast_twin(a, b, ids, tau, group, dtype=t.float64):
    """(loss, dloss/da, dloss/db) in `dtype` by autograd over the rule."""
    a = a.detach().to(dtype).clone().requires_grad_(True)
    b = b.detach().to(dtype).clone().requires_grad_(True)
    loss = contrast_loss(a, b, ids, tau, group)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def contrast_analytic(a, b, ids, tau, group):
    """The same three in float64 without autograd: softmax coefficients, then d p / d f = (I - p p^T) / |f|."""
    a, b = a.double(), b.double()
    B = ids.numel()
    fa, fb = a[ids], b[ids]
    na, nb = fa.norm(dim=1, keepdim=True), fb.norm(dim=1, keepdim=True)
    p, q = fa / na.clamp_min(FLOOR), fb / nb.clamp_min(FLOOR)
    gp, gq = t.zeros_like(p), t.zeros_like(q)
    loss = 0.0
    for g0 in range(0, B, group):
        s = slice(g0, min(g0 + group, B))
        i = ids[s]
        logit = p[s] @ q[s].T / tau
        own = t.eye(i.numel(), dtype=t.bool)
        masked = (i[None, :] == i[:, None]) & ~own
        lm = logit.masked_fill(masked, float("-inf"))
        lse = t.logsumexp(lm, dim=1)
        loss = loss + float((lse - logit.diagonal()).sum())
        c = (t.exp(lm - lse[:, None]) - own.double()) / (B * tau)
        gp[s] = c @ q[s]
        gq[s] = c.T @ p[s]

    def back(g, unit, n):
        inside = (g - unit * (unit * g).sum(dim=1, keepdim=True)) / n.clamp_min(FLOOR)
        return t.where(n >= FLOOR, inside, g / FLOOR)
    ga = t.zeros_like(a).index_add_(0, ids, back(gp, p, na))
    gb = t.zeros_like(b).index_add_(0, ids, back(gq, q, nb))
    return t.tensor(loss / B, dtype=t.float64), ga, gb


# ------------------------------------------------------------------------------------ the perturbed forward
def adjacency(row, col, n, dtype):
    """The gcn-normalised CSR of oracle/lightgcn_ref.py: (rowptr, col, val)."""
    rowptr, col_s, _ = R.sparse_tensor_csr(row, col, n, n)
    return rowptr, col_s, R.gcn_norm_csr(rowptr, col_s).to(dtype)


def perturbed_forward(e0, adj, K, eps, seed, step, layer):
    """(F, X_layer, min over layers of the smallest non-zero |Y|): the noise enters as a constant times sign(Y), detached."""
    rowptr, col, val = adj
    x, total, x_l, smallest = e0, e0, None, float("inf")
    for k in range(1, K + 1):
        y = R.spmm_torch(rowptr, col, val, x)
        yd = y.detach()
        nz = yd.abs()[yd != 0]
        if nz.numel():
            smallest = min(smallest, float(nz.min()))
        n = t.from_numpy(noise(np.arange(e0.shape[0]), e0.shape[1], k, seed, step)).to(e0.dtype)
        x = y + eps * t.sign(yd) * n
        total = total + x
        if k == layer:
            x_l = x
    return total / (K + 1), x_l, smallest


# ------------------------------------------------------------------------------------ the kernel cases
BATCHES, GROUPS, WIDTHS = (1, 31, 33, 96, 160), (32, 64), (4, 64, 256)
N_ROWS, TAU = 200, 0.15


@functools.lru_cache(maxsize=None)
def case(B, G, d, duplicated):
    """dict of B, G, d, ids [B], a [N_ROWS, d], b [N_ROWS, d], tau; seeded, built once and left unchanged.  duplicated: the
    ids come from a range of 5 (B = 33 at G = 32 leaves a last group of one slot either way); otherwise all distinct."""
    g = t.Generator().manual_seed(2000 + 7 * B + G + d + int(duplicated))
    a = 0.3 * t.randn(N_ROWS, d, generator=g)
    b = a + 0.2 * t.randn(N_ROWS, d, generator=g)           # a noisy view of the same rows: the diagonal stands out
    ids = 7 + t.randint(0, 5, (B,), generator=g) if duplicated else t.randperm(N_ROWS, generator=g)[:B]
    return dict(B=B, G=G, d=d, ids=ids, a=a, b=b, tau=TAU)


@functools.lru_cache(maxsize=None)
def reference(B, G, d, duplicated):
    """The float64 twin of a case: computed once, shared by the tests."""
    c = case(B, G, d, duplicated)
    return contrast_twin(c["a"], c["b"], c["ids"], c["tau"], c["G"])


# ------------------------------------------------------------------------------------ the main losses of the trainer test
def main_loss(f, e, n_users, users, pos, neg, lam, objective):
    """"reference" (-mean softplus(x), one negative or M) and "softmax" (sampled, over the positive and the M negatives) as the
    header states them, with the reference's L2 sum over all 2 + M rows; neg [B] or [B, M]."""
    neg = neg.reshape(users.numel(), -1)
    uf, pf, nf = f[users], f[n_users + pos], f[n_users + neg]
    sp, sn = (uf * pf).sum(-1), (uf[:, None, :] * nf).sum(-1)
    if objective == "reference":
        main = -t.nn.functional.softplus(sp[:, None] - sn).mean()
    else:
        main = (t.logsumexp(t.cat([sp[:, None], sn], dim=1), dim=1) - sp).mean()
    return main + lam * (e[users].pow(2).sum() + e[n_users + pos].pow(2).sum() + e[n_users + neg].pow(2).sum())


# ------------------------------------------------------------------------------------ the trainer's autograd twin
def train_twin(users_w, items_w, row, col, K, batches, *, lam, lr, objective, cl_weight, cl_eps, cl_tau, cl_layer, cl_group,
               seed, dtype=t.float32):
    """Steps of torch autograd + torch.optim.Adam over main_loss + cl_weight * (L_user + L_item) on the perturbed forward,
    the mirror's noise injected at (seed, step).  batches: (users, pos, neg) per step, original ids.
    Returns (losses, users table, items table, the smallest non-zero |Y| any layer of any step held)."""
    U = users_w.shape[0]
    uw = t.nn.Parameter(users_w.detach().to(dtype).clone())
    iw = t.nn.Parameter(items_w.detach().to(dtype).clone())
    opt = t.optim.Adam([uw, iw], lr=lr)
    adj = adjacency(row, col, U + items_w.shape[0], dtype)
    losses, smallest = [], float("inf")
    for step, (users, pos, neg) in enumerate(batches):
        e0 = t.cat([uw, iw])
        f, x_l, s = perturbed_forward(e0, adj, K, cl_eps, seed, step, cl_layer)
        smallest = min(smallest, s)
        loss = main_loss(f, e0, U, users, pos, neg, lam, objective)
        loss = loss + cl_weight * (contrast_loss(f, x_l, users, cl_tau, cl_group) + contrast_loss(f, x_l, U + pos, cl_tau, cl_group))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses, uw.detach(), iw.detach(), smallest
