"""CPU emulation, in float32, of the association of the table-gradient sums of mi_pinsage_project_bwd_f32 and
mi_pinsage_text_bwd_f32 (csrc/segsum.hpp): the references stable-sorted by key, the sorted list cut into pieces of 64 by
position, a run inside a piece summed from +0 in order, a run over several pieces = ((first piece's partial + the next
piece's) + ...) in piece order.  The GPU tests compare the kernels' buffers with it bit for bit."""
import numpy as np

PIECE = 64
SLOT = 1 << 40          # key = slot * SLOT + code: slot-major, as the kernels' (slot << shift) | code


def segmented_sum(keys, values):
    """keys int64 [R], values float32 [R, H] in the reference order of the call -> {key: float32 [H]}."""
    keys, values = np.asarray(keys, dtype=np.int64), np.asarray(values, dtype=np.float32)
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], values[order]
    out = {}
    for p0 in range(0, len(k), PIECE):
        p1 = min(p0 + PIECE, len(k))
        j = p0
        while j < p1:
            acc = np.zeros(v.shape[1], dtype=np.float32)
            e = j
            while e < p1 and k[e] == k[j]:
                acc = acc + v[e]                                   # one float32 addition per element, in list order
                e += 1
            key = int(k[j])
            out[key] = out[key] + acc if key in out else acc       # an earlier piece's partial comes first
            j = e
    return out


def projector_references(codes_by_slot, g):
    """Slot-major, then r: codes_by_slot[s] int64 [n] (the categorical columns, then the ids if there is an id table); the
    value of a reference is g[r]."""
    g = np.asarray(g, dtype=np.float32)
    keys = np.concatenate([s * SLOT + np.asarray(c, dtype=np.int64) for s, c in enumerate(codes_by_slot)])
    return keys, np.concatenate([g] * len(codes_by_slot))


def text_references(columns, rows, g):
    """Pairs in (column, r) order, then the position in the bag: columns[c] = (ptr, tok) over the catalogue, rows int64 [n]
    the item of each row of g; the value is g[r] / float32(len), one correctly rounded float32 division per element."""
    g = np.asarray(g, dtype=np.float32)
    keys, values = [], []
    for c, (ptr, tok) in enumerate(columns):
        ptr, tok = np.asarray(ptr, dtype=np.int64), np.asarray(tok, dtype=np.int64)
        for r, item in enumerate(np.asarray(rows, dtype=np.int64)):
            p0, p1 = int(ptr[item]), int(ptr[item + 1])
            if p1 > p0:
                keys.append(c * SLOT + tok[p0:p1])
                values.append(np.repeat((g[r] / np.float32(p1 - p0))[None, :], p1 - p0, 0))
    if not keys:
        return np.zeros(0, dtype=np.int64), np.zeros((0, g.shape[1]), dtype=np.float32)
    return np.concatenate(keys), np.concatenate(values)


def expected_tables(sums, slot, like, sentinel):
    """The buffer of table `slot`: `sentinel` everywhere but the rows `sums` holds for it.  like: float32 [rows, H]."""
    want = np.full(like.shape, sentinel, dtype=np.float32)
    for key, row in sums.items():
        if key // SLOT == slot:
            want[key % SLOT] = row
    return want
