"""Record the bits of the one-negative loss entry (ops.bpr_fwd_bwd) and of the default trainer step into
tests/golden/bpr_entry_bits.json: raw fp32 bits of every loss, SHA-256 of the bytes of g_final, reg_w and the table.

tests/test_gpu_objectives.py compares both loss entries and the default step with this file.  The committed file was
recorded at the commit it names, the last one whose one-negative entry had a host body of its own; a run on a later tree
records that tree and is worth a diff against the committed file, nothing else.  The batches below are the test's
(_small_batch, _model_and_graph, _run): change neither side alone.

It also writes tests/golden/loss_path_bits.json: the same for every other loss path (ops.rank_loss_fwd_bwd over objectives, M,
D and node map on four kinds of batch; ops.inbatch_softmax_fwd_bwd over the twin's shapes and two more), recorded at the
commit that file names, before the paths shared csrc/refsum.hpp.  Both GPU test files take these cases and their records
from the functions below.

And tests/golden/tile_loss_bits.json: the full-catalogue softmax (ops.full_softmax_fwd_bwd) and the noise-view contrastive
term (ops.contrastive_fwd_bwd) on the shapes of their twins, recorded at the commit that file names, before they shared
csrc/loss_tiles.hpp with the in-batch softmax.  tests/test_gpu_full_softmax.py and tests/test_gpu_contrastive.py take their
cases and records from here in the same way.
    python3 tools/record_loss_bits.py --commit <short hash of the tree that runs> [--out tests/golden/bpr_entry_bits.json]
                                      [--paths-out tests/golden/loss_path_bits.json]
                                      [--tiles-out tests/golden/tile_loss_bits.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the batches and shapes of the tests
import torch as t
from laplace_amd import ops
from laplace_amd.interactions import Interactions
from laplace_amd.model.lightgcn import LightGCN
from laplace_amd.trainer import LightGCNTrainer

DEV = "cuda"
DIMS = (32, 64, 100, 128, 200, 512)
LOSS_ONLY_DIMS = (64, 128)
G_SCALES = (1.0, 1.0 / 3)


def bits(x) -> str:
    """The fp32 value's bit pattern, 8 hex digits."""
    return f"{t.as_tensor(x, dtype=t.float32).reshape(-1)[:1].cpu().view(t.int32).item() & 0xFFFFFFFF:08x}"


def digest(x: t.Tensor) -> str:
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def small_batch(B, D, seed, U, I):
    g = t.Generator().manual_seed(seed)
    final = t.randn(U + I, D, generator=g) * 0.3
    e0 = t.randn(U + I, D, generator=g)
    users, pos = t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g)
    neg = t.randint(0, I, (B, 1), generator=g)
    return final, e0, users, pos, neg[:, 0].contiguous()


def entry_cases():
    B, lam, U, I = 300, 1e-3, 40, 25
    full, loss_only = {}, {}
    for D in DIMS:
        final, e0, users, pos, neg = small_batch(B, D, D, U, I)
        ud, pd, nd, e0d = users.to(DEV), pos.to(DEV), neg.to(DEV), e0.to(DEV)
        for with_map in (False, True):
            src, gmap, rows_n = final.to(DEV), None, U + I
            if with_map:
                gmap, nodes, cnt = ops.batch_nodes(ud, pd, nd, U, U + I)
                rows_n = 3 * B
                src = t.zeros(rows_n, D, device=DEV)
                src[: int(cnt[0])] = final.to(DEV)[nodes[: int(cnt[0])].long()]
            for gi, g_scale in enumerate(G_SCALES):
                gf, rw = t.zeros(rows_n, D, device=DEV), t.zeros(U + I, device=DEV)
                loss = ops.bpr_fwd_bwd(ud, pd, nd, src, e0d, U, lam, g_final=gf, reg_w=rw, g_scale=g_scale, node_map=gmap)
                full[f"D{D}_map{int(with_map)}_gscale{gi}"] = {"loss_bits": bits(loss), "g_final_sha256": digest(gf),
                                                               "reg_w_sha256": digest(rw)}
            if D in LOSS_ONLY_DIMS:   # reg_w of this form comes from float atomics: the loss alone
                rw = t.zeros(U + I, device=DEV)
                loss = ops.bpr_fwd_bwd(ud, pd, nd, src, e0d, U, lam, reg_w=rw, node_map=gmap)
                loss_only[f"D{D}_map{int(with_map)}"] = {"loss_bits": bits(loss)}
    return full, loss_only


def default_trainer():
    U, I, E, D, K, B = 900, 500, 15000, 64, 3, 512
    g = t.Generator().manual_seed(41)
    ei = t.stack([t.randint(0, U, (E,), generator=g), t.randint(0, I, (E,), generator=g)])
    t.manual_seed(41)
    model = LightGCN(U, I, embedding_dim=D, num_iterations=K)
    inter = Interactions(ei, U, I)
    adj = inter.adjacency("bipartite")
    model.to(DEV)
    tr = LightGCNTrainer(model, adj.to(DEV), inter.to(DEV), lr=1e-3, Lambda=1e-4, batch_size=B, seed=9)
    losses = [bits(tr.step()) for _ in range(3)]
    tr.finish()
    return {"loss_bits": losses, "table_sha256": digest(tr.table)}


# ---- every loss path against its own past: tests/golden/loss_path_bits.json --------------------------------------------------
# The M-negative entries (ops.rank_loss_fwd_bwd, logq included) and the in-batch softmax, whose gradient passes all end in
# the sorted-reference segmented sum of csrc/refsum.hpp.  tests/test_gpu_objectives.py and tests/test_gpu_inbatch_softmax.py
# take the cases and the records from the functions below, so the file and the tests cannot drift apart.
RANK_OBJECTIVES = ("reference", "bpr", "softmax", "softmax+logq")
RANK_NEGS = (1, 4, 16)
RANK_DIMS = (32, 100, 200, 512)          # 1, 2, 4, 8 floats of a row per lane, with ragged tails
# batch kind -> (B, U, I, the M it is run at); n_ref = (2 + M) B
RANK_BATCHES = {"dense": (300, 5, 6, RANK_NEGS),      # 11 nodes: every run crosses chunk borders, chunks lie wholly inside runs
                "sparse": (96, 4000, 3000, RANK_NEGS),  # runs mostly of one; 288 references at M = 1: a ragged last chunk
                "one_chunk": (16, 5, 6, (2,)),        # n_ref = 64: one full chunk
                "chunk_plus_one": (13, 5, 6, (3,))}   # n_ref = 65: one chunk and one reference
INBATCH_LAMS = (0.0, 1e-2)               # LAMS of tests/test_gpu_inbatch_softmax.py
# (B, G, d, users, items) beside inbatch_softmax_twin.SHAPES: 2B = 64, one full chunk, and one reference more; the smallest group
INBATCH_EXTRA_SHAPES = ((32, 32, 16, 5, 6), (33, 32, 16, 5, 6))


def rank_cases(kind, objective):
    """The cases of one batch kind and objective: dicts of kind, objective, M, D, with_map and their key in the file."""
    return [dict(kind=kind, objective=objective, M=M, D=D, with_map=with_map,
                 key=f"{kind}_{objective}_M{M}_D{D}_map{int(with_map)}")
            for M in RANK_BATCHES[kind][3] for D in RANK_DIMS for with_map in (False, True)]


def rank_record(c):
    """Loss bits, digests of g_final and reg_w, and the loss bits of the loss-only form (no g_final, no reg_w) of case c."""
    from test_gpu_objectives import _small_batch
    B, U, I, _ = RANK_BATCHES[c["kind"]]
    M, D = c["M"], c["D"]
    _, _, final, e0, users, pos, neg = _small_batch(B, M, D, seed=1000 * M + D, U=U, I=I)
    objective, logq = c["objective"], None
    if objective == "softmax+logq":
        objective = "softmax"
        logq = t.log(0.1 * t.rand(I, generator=t.Generator().manual_seed(D + M)) + 1e-4).to(DEV)
    ud, pd, nd, e0d = users.to(DEV), pos.to(DEV), neg.to(DEV), e0.to(DEV)
    src, gmap, rows_n = final.to(DEV), None, U + I
    if c["with_map"]:
        gmap, nodes, cnt = ops.batch_nodes(ud, pd, nd, U, U + I)
        rows_n = (2 + M) * B
        src = t.zeros(rows_n, D, device=DEV)
        src[: int(cnt[0])] = final.to(DEV)[nodes[: int(cnt[0])].long()]
    gf, rw = t.zeros(rows_n, D, device=DEV), t.zeros(U + I, device=DEV)
    kw = dict(objective=objective, node_map=gmap, logq=logq)
    loss = ops.rank_loss_fwd_bwd(ud, pd, nd, src, e0d, U, 1e-3, g_final=gf, reg_w=rw, g_scale=1.0 / 3, **kw)
    only = ops.rank_loss_fwd_bwd(ud, pd, nd, src, e0d, U, 1e-3, **kw)
    return {"loss_bits": bits(loss), "g_final_sha256": digest(gf), "reg_w_sha256": digest(rw), "loss_only_bits": bits(only)}


def inbatch_shapes():
    import inbatch_softmax_twin as T
    return len(T.SHAPES) + len(INBATCH_EXTRA_SHAPES)


def _inbatch_inputs(i):
    """Case i of inbatch_softmax_twin.cases(), or the extra shape that follows them (skewed ids: long runs)."""
    import inbatch_softmax_twin as T
    if i < len(T.SHAPES):
        return T.cases()[i]
    B, G, d, U, I = INBATCH_EXTRA_SHAPES[i - len(T.SHAPES)]
    g = t.Generator().manual_seed(2000 + i)
    final, e0 = 0.3 * t.randn(U + I, d, generator=g), t.randn(U + I, d, generator=g)
    logq = t.log(0.1 * t.rand(I, generator=g) + 1e-4)
    users, pos = t.randint(0, U, (B,), generator=g), t.randint(0, I, (B,), generator=g)
    return dict(B=B, G=G, d=d, U=U, I=I, final=final, e0=e0, logq=logq, users=users, pos=pos)


def inbatch_cases(i):
    return [dict(i=i, lam=lam, with_logq=with_logq, with_map=with_map,
                 key=f"shape{i}_lam{li}_logq{int(with_logq)}_map{int(with_map)}")
            for li, lam in enumerate(INBATCH_LAMS) for with_logq in (False, True) for with_map in (False, True)]


def inbatch_record(c):
    s = _inbatch_inputs(c["i"])
    U, I, d, B = s["U"], s["I"], s["d"], s["B"]
    ud, pd, e0d = s["users"].to(DEV), s["pos"].to(DEV), s["e0"].to(DEV)
    src, gmap, rows_n = s["final"].to(DEV), None, U + I
    if c["with_map"]:
        gmap, nodes, cnt = ops.batch_nodes(ud, pd, pd, U, U + I)   # the node set of (users, pos): neg aliased to pos
        rows_n = 2 * B
        src = t.zeros(rows_n, d, device=DEV)
        src[: int(cnt[0])] = s["final"].to(DEV)[nodes[: int(cnt[0])].long()]
    gf, rw = t.zeros(rows_n, d, device=DEV), t.zeros(U + I, device=DEV)
    kw = dict(group=s["G"], logq=s["logq"].to(DEV) if c["with_logq"] else None, node_map=gmap)
    loss = ops.inbatch_softmax_fwd_bwd(ud, pd, src, e0d, U, c["lam"], g_final=gf, reg_w=rw, g_scale=1.0 / 3, **kw)
    only = ops.inbatch_softmax_fwd_bwd(ud, pd, src, e0d, U, c["lam"], **kw)
    return {"loss_bits": bits(loss), "g_final_sha256": digest(gf), "reg_w_sha256": digest(rw), "loss_only_bits": bits(only)}


def loss_paths():
    rank = {c["key"]: rank_record(c) for kind in RANK_BATCHES for o in RANK_OBJECTIVES for c in rank_cases(kind, o)}
    inb = {c["key"]: inbatch_record(c) for i in range(inbatch_shapes()) for c in inbatch_cases(i)}
    return rank, inb


# ---- the losses on 32 x 32 score tiles against their own past: tests/golden/tile_loss_bits.json -------------------------------
# The full-catalogue softmax and the noise-view contrastive term, which share the tile routines of csrc/loss_tiles.hpp with
# the in-batch softmax above.  tests/test_gpu_full_softmax.py and tests/test_gpu_contrastive.py take the cases and the
# records from the functions below.
FULL_LAMS = (0.0, 1e-2)                  # LAMS of tests/test_gpu_full_softmax.py


def full_softmax_shapes():
    import full_softmax_twin as T
    return len(T.SHAPES)


def full_softmax_cases(i):
    return [dict(i=i, lam=lam, key=f"shape{i}_lam{li}") for li, lam in enumerate(FULL_LAMS)]


def full_softmax_record(c):
    import full_softmax_twin as T
    s = T.cases()[c["i"]]
    U, I, d = s["U"], s["I"], s["d"]
    ud, pd, fd, e0d = s["users"].to(DEV), s["pos"].to(DEV), s["final"].to(DEV), s["e0"].to(DEV)
    gf, rw = t.zeros(U + I, d, device=DEV), t.zeros(U + I, device=DEV)
    loss = ops.full_softmax_fwd_bwd(ud, pd, fd, e0d, U, c["lam"], g_final=gf, reg_w=rw, g_scale=1.0 / 3)
    only = ops.full_softmax_fwd_bwd(ud, pd, fd, e0d, U, c["lam"])
    return {"loss_bits": bits(loss), "g_final_sha256": digest(gf), "reg_w_sha256": digest(rw), "loss_only_bits": bits(only)}


def contrastive_cases(B):
    """The cases of one batch size of contrastive_emulation: every group, width and kind of ids."""
    import contrastive_emulation as E
    return [dict(B=B, G=G, d=d, duplicated=dup, key=f"B{B}_G{G}_d{d}_dup{int(dup)}")
            for G in E.GROUPS for d in E.WIDTHS for dup in (False, True)]


def contrastive_record(c):
    import contrastive_emulation as E
    s = E.case(c["B"], c["G"], c["d"], c["duplicated"])
    a, b, ids = s["a"].to(DEV), s["b"].to(DEV), s["ids"].to(DEV)
    g_a, g_b = t.zeros_like(a), t.zeros_like(b)
    loss = ops.contrastive_fwd_bwd(ids, a, b, tau=E.TAU, group=c["G"], g_a=g_a, g_b=g_b, g_scale_a=1.0 / 3, g_scale_b=1.0)
    only = ops.contrastive_fwd_bwd(ids, a, b, tau=E.TAU, group=c["G"])
    return {"loss_bits": bits(loss), "g_a_sha256": digest(g_a), "g_b_sha256": digest(g_b), "loss_only_bits": bits(only)}


def tile_losses():
    import contrastive_emulation as E
    full = {c["key"]: full_softmax_record(c) for i in range(full_softmax_shapes()) for c in full_softmax_cases(i)}
    con = {c["key"]: contrastive_record(c) for B in E.BATCHES for c in contrastive_cases(B)}
    return full, con


def write_json(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="short hash of the tree that runs; written into the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bpr_entry_bits.json"))
    ap.add_argument("--paths-out", default=os.path.join(ROOT, "tests", "golden", "loss_path_bits.json"))
    ap.add_argument("--tiles-out", default=os.path.join(ROOT, "tests", "golden", "tile_loss_bits.json"))
    args = ap.parse_args()
    full_sm, con = tile_losses()
    write_json(args.tiles_out, {
        "recorded_at_commit": args.commit,
        "what": "ops.full_softmax_fwd_bwd (full_softmax: shape of full_softmax_twin.SHAPES, lam; g_scale 1/3) and "
                "ops.contrastive_fwd_bwd (contrastive: B, G, d, duplicated ids of contrastive_emulation; tau 0.15, gradient "
                "tables zero on entry, g_scale_a 1/3, g_scale_b 1) on the cases of tools/record_loss_bits.py.  fp32 bit "
                "patterns in hex (loss, and the loss of the loss-only form), SHA-256 of the bytes of g_final and reg_w, "
                "or of g_a and g_b.",
        "full_softmax": full_sm, "contrastive": con})
    print(f"{len(full_sm)} full-softmax and {len(con)} contrastive cases -> {args.tiles_out}")
    rank, inb = loss_paths()
    write_json(args.paths_out, {
        "recorded_at_commit": args.commit,
        "what": "ops.rank_loss_fwd_bwd (rank: batch kind, objective, M, D, node map; lam 1e-3, g_scale 1/3) and "
                "ops.inbatch_softmax_fwd_bwd (in_batch: shape, lam, logq, node map; g_scale 1/3) on the cases of "
                "tools/record_loss_bits.py.  fp32 bit patterns in hex (loss, and the loss of the loss-only form), SHA-256 "
                "of the bytes of g_final and reg_w.",
        "rank": rank, "in_batch": inb})
    print(f"{len(rank)} rank and {len(inb)} in-batch cases -> {args.paths_out}")
    full, loss_only = entry_cases()
    out = {"recorded_at_commit": args.commit,
           "what": "ops.bpr_fwd_bwd on _small_batch(300, 1, D, seed=D, U=40, I=25), lam 1e-3, g_scale 1 and 1/3 "
                   "(gscale0 / gscale1), without and with node map; its loss-only form; three default trainer steps of "
                   "_run('reference', 1, steps=3).  fp32 bit patterns in hex, SHA-256 of the arrays' bytes.",
           "entry": full, "entry_loss_only": loss_only, "default_trainer": default_trainer()}
    write_json(args.out, out)
    print(f"{len(full)} + {len(loss_only)} entry cases and the default trainer's three steps -> {args.out}")
