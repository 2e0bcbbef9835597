"""numpy mirror of the popularity-weighted negative sampler (mi_sample_bpr_batch_pop) and the float64 twin of the
logQ-corrected sampled softmax, as include/laplace_hip.h states them.  Test infrastructure: the mirror takes the
PRODUCT's cum (the table builder is checked by properties in tests/test_neg_sampling_cpu.py), draws on oracle/philox.py
and is vectorised over attempts: every pending (slot, m) of an attempt is drawn in one Philox call."""
import numpy as np
import torch as t

from oracle.philox import philox4x32

TAG_EDGE, TAG_NEG = 0x45444745, 0x4E454721
MAX_ATTEMPTS = 4096
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def cum_u32(table):
    """The uint32 words of a NegativeTable's cum (held as int32 of the same bits), as uint64 for the arithmetic below."""
    return table.cum.cpu().numpy().view(np.uint32).astype(np.uint64)


def _key(seed, step):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF


def draw(cum, e, tt, m, seed, step):
    """The candidate of edge e, attempt tt, negative m (arrays or scalars, broadcast): r = ((c0 << 32) | c1) % total of the
    counter (e, tt | m << 16) of the NEG! stream, then the smallest i with cum[i] > r."""
    k0, k1, s0, s1 = _key(seed, step)
    e = np.asarray(e, dtype=np.uint64)
    c1 = np.asarray(tt, dtype=np.uint64) | (np.asarray(m, dtype=np.uint64) << np.uint64(16))
    q = philox4x32(e & _U32, c1, s0, s1 ^ TAG_NEG, k0, k1)
    r = ((q[0] << _S32) | q[1]) % np.uint64(cum[-1])
    return np.searchsorted(cum, r, side="right").astype(np.int64)


def edges(batch, nnz, seed, step, edges_in_order=False):
    """The edge of every slot: the uniform samplers' EDGE stream."""
    if edges_in_order:
        return np.arange(batch, dtype=np.int64)
    k0, k1, s0, s1 = _key(seed, step)
    b = np.arange(batch, dtype=np.uint64)
    r = philox4x32(b & _U32, b >> _S32, s0, s1 ^ TAG_EDGE, k0, k1)
    return (((r[0] << _S32) | r[1]) % np.uint64(nnz)).astype(np.int64)


def sample(rowptr, col, batch, n_neg, cum, seed, step, edges_in_order=False):
    """(users [B], pos [B], neg [B, n_neg]) int64 of mi_sample_bpr_batch_pop.  rowptr / col: the sorted CSR of the user
    rows; cum: uint32-valued array of the table."""
    rp, c = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    cum = np.asarray(cum, dtype=np.uint64)
    n_rows, nnz = rp.shape[0] - 1, c.shape[0]
    row_of_edge = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rp))
    e = edges(batch, nnz, seed, step, edges_in_order)
    users, pos = row_of_edge[e], c[e]
    neg = np.zeros((batch, n_neg), dtype=np.int64)
    if int(cum[-1]) == 0:
        return users, pos, neg
    width = int(max(c.max() + 1, cum.shape[0])) + 1
    held = np.sort(row_of_edge * width + c)            # (user, item) keys of the interactions
    slot, m = np.divmod(np.arange(batch * n_neg, dtype=np.int64), n_neg)
    for tt in range(MAX_ATTEMPTS):
        cand = draw(cum, e[slot], tt, m, seed, step)
        neg[slot, m] = cand                              # the last candidate stays
        keys = users[slot] * width + cand
        at = np.minimum(np.searchsorted(held, keys), held.shape[0] - 1)
        hit = held[at] == keys
        if not hit.any():
            break
        slot, m = slot[hit], m[hit]
    return users, pos, neg


def twin_softmax_logq(uf, u0, pf, p0, nf, n0, lam, pos_logq, neg_logq):
    """The corrected sampled softmax on gathered blocks (nf / n0 [B, M, D], neg_logq [B, M]) in the dtype of the blocks:
    (1/B) sum_b [ logsumexp(s+ - lq+, s-_1 - lq-_1, ..) - (s+ - lq+) ] + lam * sum of squares of the layer-0 rows."""
    sp = (uf * pf).sum(-1) - pos_logq.to(uf.dtype)
    sn = (uf[:, None, :] * nf).sum(-1) - neg_logq.to(uf.dtype)
    main = (t.logsumexp(t.cat([sp[:, None], sn], dim=1), dim=1) - sp).mean()
    return main + lam * (u0.pow(2).sum() + p0.pow(2).sum() + n0.pow(2).sum())
