"""Record the bits of the one-negative loss entry (ops.bpr_fwd_bwd) and of the default trainer step into
tests/golden/bpr_entry_bits.json: raw fp32 bits of every loss, SHA-256 of the bytes of g_final, reg_w and the table.

tests/test_gpu_objectives.py compares both loss entries and the default step with this file.  The committed file was
recorded at the commit it names, the last one whose one-negative entry had a host body of its own; a run on a later tree
records that tree and is worth a diff against the committed file, nothing else.  The batches below are the test's
(_small_batch, _model_and_graph, _run): change neither side alone.
    python3 tools/record_loss_bits.py --commit <short hash of the tree that runs> [--out tests/golden/bpr_entry_bits.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="short hash of the tree that runs; written into the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bpr_entry_bits.json"))
    args = ap.parse_args()
    full, loss_only = entry_cases()
    out = {"recorded_at_commit": args.commit,
           "what": "ops.bpr_fwd_bwd on _small_batch(300, 1, D, seed=D, U=40, I=25), lam 1e-3, g_scale 1 and 1/3 "
                   "(gscale0 / gscale1), without and with node map; its loss-only form; three default trainer steps of "
                   "_run('reference', 1, steps=3).  fp32 bit patterns in hex, SHA-256 of the arrays' bytes.",
           "entry": full, "entry_loss_only": loss_only, "default_trainer": default_trainer()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(full)} + {len(loss_only)} entry cases and the default trainer's three steps -> {args.out}")
