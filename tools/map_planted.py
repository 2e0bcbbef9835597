"""MAP@12 on a planted-structure synthetic graph (synthetic.SyntheticSpec.communities): layer-0 predictor (the
reference's, F8) vs propagated embeddings vs the popularity predictor, at checkpoints of the training run.
    python3 tools/map_planted.py --users 50000 --items 5000 --edges 1000000 --batch 16384 --lr 0.01 --steps 50,100,200
--objective / --n-neg choose the training loss (trainer.LightGCNTrainer); --predictor names the figure reported as
"map_at_12": the layer-0 tables (default) or the propagated embeddings the loss trains.
--model als: the same protocol with iALS (als.ImplicitALS; --alpha, --reg) in the trainer's place, scored after each epoch count
of --als-epochs; --als-solver block (--als-block, --als-sweeps) trains it with the block row solver, the only one for
--dim > 128; --als-reg-power NU trains it with the frequency-scaled regulariser reg * (n_cols + sum_e a_e)^NU (--reg must be
retuned with NU: it multiplies a factor in the thousands at NU = 1).  --init als: LightGCN's tables start from the iALS factors after max(--als-epochs) epochs.  --seed moves the
model's initial tables and the trainer's sampler (the graph and the held-out pairs stay the recipe's).  Every line also carries
map@12, mrr and recall@100 of the full-catalogue ranks (utils.metrics_lightgcn.full_rank_metrics) of the held-out pairs."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as t
from dataclasses import replace
import bench
from laplace_amd import synthetic as S
from laplace_amd.interactions import Interactions
from laplace_amd.model.lightgcn import LightGCN
from laplace_amd.trainer import LightGCNTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=943)
ap.add_argument("--items", type=int, default=1682)
ap.add_argument("--edges", type=int, default=100000)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--lr", type=float, default=1e-2)
ap.add_argument("--communities", type=int, default=8)
ap.add_argument("--mix", type=float, default=0.85)
ap.add_argument("--steps", default="0,50,100,200,400")
ap.add_argument("--eval-users", type=int, default=20000)
ap.add_argument("--deg-min", type=int, default=1)
ap.add_argument("--objective", default="reference", choices=["reference", "bpr", "softmax"])
ap.add_argument("--n-neg", type=int, default=1)
ap.add_argument("--predictor", default="layer0", choices=["layer0", "propagated"])
ap.add_argument("--model", default="lightgcn", choices=["lightgcn", "als"])
ap.add_argument("--init", default="random", choices=["random", "als"])
ap.add_argument("--als-epochs", default="1,3,5,10")
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--reg", type=float, default=20.0)
ap.add_argument("--als-solver", default="cholesky", choices=["cholesky", "block"])
ap.add_argument("--als-block", type=int, default=16)
ap.add_argument("--als-sweeps", type=int, default=1)
ap.add_argument("--als-reg-power", type=float, default=0.0)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
spec = S.SyntheticSpec(args.users, args.items, args.edges, seed=5, communities=args.communities, community_mix=args.mix,
                       deg_min=args.deg_min, deg_max=min(2000, args.items // 2))
ei = S.generate(spec)
held = S.heldout_edges(spec, ei, args.eval_users).to("cuda")
from laplace_amd.als import ImplicitALS
from laplace_amd.run_pipeline_lightgcn import propagated_embeddings
from laplace_amd.utils.metrics_lightgcn import get_full_rank_metrics_lightgcn
inter = Interactions(ei.to("cuda"), args.users, args.items)
als_epochs = [int(x) for x in args.als_epochs.split(",")]


def full_rank(m, embeddings=None):
    r = get_full_rank_metrics_lightgcn(m, held, [inter.edge_index], ks=(12, 100), embeddings=embeddings)
    return {k: round(r[k], 4) for k in ("map@12", "mrr", "recall@100")}


def popularity():
    deg = t.bincount(inter.edge_index[1], minlength=args.items).to(t.float32)
    ue, ie = t.zeros(args.users, 4, device="cuda"), t.zeros(args.items, 4, device="cuda")
    ue[:, 0], ie[:, 0] = 1.0, deg
    return full_rank(None, (ue, ie))


als = None
if args.model == "als" or args.init == "als":
    als = ImplicitALS(args.users, args.items, dim=args.dim, alpha=args.alpha, reg=args.reg, seed=args.seed,
                      solver=args.als_solver, block=args.als_block, block_sweeps=args.als_sweeps,
                      reg_power=args.als_reg_power).to("cuda")
    done = 0
    for cp in (als_epochs if args.model == "als" else [max(als_epochs)]):
        als.fit(inter, cp - done)
        done = cp
        if args.model == "als":
            print(cp, json.dumps({"model": "als", "solver": args.als_solver, "dim": args.dim, "seed": args.seed, "reg": args.reg,
                                  "reg_power": args.als_reg_power, **full_rank(als),
                                  "objective": round(als.objective(inter), 2)}), flush=True)
if args.model == "als":
    print("popularity", json.dumps(popularity()), flush=True)
    sys.exit(0)
t.manual_seed(args.seed)
model = LightGCN(args.users, args.items, args.dim, args.layers).to("cuda")
if als is not None:
    with t.no_grad():
        model.users_emb.weight.copy_(als.users_emb.weight)
        model.items_emb.weight.copy_(als.items_emb.weight)
adj = inter.adjacency("bipartite")
tr = LightGCNTrainer(model, adj, inter, lr=args.lr, Lambda=1e-6, batch_size=args.batch, seed=7 + args.seed,
                     objective=args.objective, n_neg=args.n_neg)
done = 0
for cp in [int(x) for x in args.steps.split(",")]:
    out = bench.map_at_12(model, tr, inter, held, cp - done)
    done = cp
    out["map_at_12"] = out["value"] if args.predictor == "layer0" else out["propagated_embeddings_map_at_12"]
    out["loss"] = float(tr.loss)
    line = {k: round(v, 4) if isinstance(v, float) else v for k, v in out.items() if "map" in k or k in ("value", "loss")}
    line["full_rank_layer0"] = full_rank(model)                       # map_at_12 left the model's rows under their original ids
    line["full_rank_propagated"] = full_rank(model, propagated_embeddings(model, adj))
    print(cp, json.dumps(line), flush=True)
