"""Record what the two LightGCN trainers (trainer.LightGCNTrainer, dist.ShardedLightGCNTrainer at world 1) compute and launch
into tests/golden/trainer_path_bits.json.

For every case, four steps with decay_lr() after the second: the raw fp32 bits of each step's loss, one SHA-256 over the bytes of
`table`, `m` and `v` after finish(), the SHA-256 of sample() before the first step, and for steps 1 and 2 the sequence of
laplace_amd.ops calls the step made: the function's name, the sorted names of its keyword arguments that are not None and, for
spmm, the trainer attribute(s) that hold the adjacency it got.  The calls are seen by wrappers set on the module's functions
(the `setattr` the caller hands in: pytest's monkeypatch.setattr in the tests), so what is recorded is what the module was asked
to launch, whoever asked.  Equal sequences are written once, under "sequences", and named by the cases.

The inputs are integer formulas (graph() and table() below; no RNG), and every case runs twice: a case whose two runs differ in
any bit is not written, since the file rests on the step being bitwise reproducible.  The committed file was recorded at the
commit it names, the last one at which each trainer carried its own copy of the host logic they share;
tests/test_gpu_lightgcn.py recomputes every case and compares for equality.  The tests take their cases and their records from
cases() and record() below, so the file and the tests cannot drift apart.
    python3 tools/record_trainer_bits.py --commit <short hash of the tree that runs> [--out tests/golden/trainer_path_bits.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch as t

DEV = "cuda"
U, I, D = 257, 131, 32
BATCH, GROUP, M = 64, 32, 4
STEPS, DECAY_AFTER, CALL_STEPS = 4, 2, 2
WRAPPED = ("spmm", "gather_rows", "scatter_rows", "batch_nodes", "sample_bpr_batch", "rank_loss_fwd_bwd", "bpr_fwd_bwd",
           "inbatch_softmax_fwd_bwd", "adam_step")
ADJACENCIES = ("adj_fwd", "adj_bwd", "a_users", "a_items")
# the single-device trainer's objective cases: key -> constructor arguments
OBJECTIVES = {"bpr4": dict(objective="bpr", n_neg=M), "softmax4": dict(objective="softmax", n_neg=M),
              "softmax1": dict(objective="softmax", n_neg=1),
              "pop_softmax4": dict(objective="softmax", n_neg=M, negatives="popularity"),
              "pop_reference1": dict(negatives="popularity"),
              "softmax4_logq": dict(objective="softmax", n_neg=M, logq_correction=True),
              "inbatch_logq": dict(objective="softmax", negatives="in_batch", in_batch_group=GROUP),
              "inbatch": dict(objective="softmax", negatives="in_batch", in_batch_group=GROUP, logq_correction=False)}
SHARDED_OBJECTIVES = {"bpr4": OBJECTIVES["bpr4"], "softmax4": OBJECTIVES["softmax4"]}


def bits(x) -> str:
    """The fp32 value's bit pattern, 8 hex digits."""
    return f"{t.as_tensor(x, dtype=t.float32).reshape(-1)[:1].cpu().view(t.int32).item() & 0xFFFFFFFF:08x}"


def digest_all(tensors) -> str:
    """One SHA-256 over the bytes of every tensor, in their order."""
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def graph() -> t.Tensor:
    """User u buys item 0 and the items (7u + 13j) % 130 + 1 for j < 3 + u % 5: item 0 has 257 entries, one more than
    ops.DEFAULT_CHUNK, so its row is a split row of the plan and of the row_list launches."""
    users, items = [], []
    for u in range(U):
        mine = [0] + [(7 * u + 13 * j) % 130 + 1 for j in range(3 + u % 5)]
        users += [u] * len(mine)
        items += mine
    return t.tensor([users, items], dtype=t.int64)


def table() -> t.Tensor:
    r, c = t.arange(U + I, dtype=t.int64)[:, None], t.arange(D, dtype=t.int64)[None, :]
    return ((31 * r + 17 * c) % 97 - 48).to(t.float32) / 480


def cases():
    out = []
    for kind in ("single", "sharded"):
        for sb in (True, False):
            for K in (0, 1, 3):
                for ro in (False, True):
                    out.append(dict(kind=kind, K=K, kw=dict(sparse_batch=sb, reorder=ro), key=f"{kind}_sparse{int(sb)}_K{K}_reorder{int(ro)}"))
    out += [dict(kind="single", K=K, kw=dict(fuse_adam=False), key=f"single_unfused_adam_K{K}") for K in (1, 3)]
    for name, kw in OBJECTIVES.items():
        out.append(dict(kind="single", K=3, kw=dict(kw), key=f"single_{name}"))
        out += [dict(kind="single", K=3, kw=dict(kw, sparse_batch=sb, reorder=True), key=f"single_{name}_sparse{int(sb)}_reorder1")
                for sb in (True, False)]
    out += [dict(kind="single", K=3, kw=dict(reference_sampler_quirks=True, reorder=False), key="single_sampler_quirks"),
            dict(kind="single", K=3, kw=dict(neg_range=I - 1, reorder=False), key="single_neg_range130")]
    for name, kw in SHARDED_OBJECTIVES.items():
        out += [dict(kind="sharded", K=3, kw=dict(kw, sparse_batch=sb, reorder=True), key=f"sharded_{name}_sparse{int(sb)}_reorder1")
                for sb in (True, False)]
    # step(batch): the batch, in original ids, is what a twin's sample() gives; the in-batch trainer is fed (users, pos)
    for kind in ("single", "sharded"):
        out += [dict(kind=kind, K=3, kw=dict(sparse_batch=sb, reorder=True), feed=3, key=f"{kind}_fed_batch_sparse{int(sb)}")
                for sb in (True, False)]
    out += [dict(kind="single", K=3, kw=dict(OBJECTIVES["softmax4"], reorder=True), feed=3, key="single_fed_batch_softmax4"),
            dict(kind="single", K=3, kw=dict(OBJECTIVES["inbatch_logq"], reorder=True), feed=2, key="single_fed_batch_inbatch")]
    return out


def _trainer(c):
    from laplace_amd.dist import ShardedLightGCNTrainer
    from laplace_amd.interactions import Interactions
    from laplace_amd.model.lightgcn import LightGCN
    from laplace_amd.trainer import LightGCNTrainer
    model = LightGCN(U, I, embedding_dim=D, num_iterations=c["K"])
    e0 = table()
    with t.no_grad():
        model.users_emb.weight.copy_(e0[:U])
        model.items_emb.weight.copy_(e0[U:])
    model.to(DEV)
    inter = Interactions(graph().to(DEV), U, I)
    hyper = dict(lr=1e-2, Lambda=1e-4, batch_size=BATCH, seed=5)
    if c["kind"] == "sharded":
        return ShardedLightGCNTrainer(model, inter, **hyper, **c["kw"])
    return LightGCNTrainer(model, inter.adjacency("bipartite"), inter, **hyper, **c["kw"])


class Calls:
    """Wrappers on the WRAPPED functions of laplace_amd.ops, set once with the caller's setattr(object, name, value), whose to
    undo they are.  While `log` is a list, every call is appended to it."""
    def __init__(self, setattr):
        from laplace_amd import ops
        self.log, self.trainer = None, None
        for name in WRAPPED:
            setattr(ops, name, self._wrapper(name, getattr(ops, name)))

    def _wrapper(self, name, fn):
        def call(*a, **kw):
            if self.log is not None:
                what = name
                if name == "spmm":
                    what += "[" + "=".join(k for k in ADJACENCIES if getattr(self.trainer, k, None) is a[0]) + "]"
                self.log.append(what + "(" + ",".join(sorted(k for k, v in kw.items() if v is not None)) + ")")
            return fn(*a, **kw)
        return call


def _run(c, calls: Calls) -> dict:
    tr = calls.trainer = _trainer(c)
    twin = _trainer(c) if "feed" in c else None
    out = {"sample_sha256": digest_all(tr.sample()), "loss_bits": [], "calls": []}
    for s in range(STEPS):
        batch = None
        if twin is not None:
            batch = tuple(twin.sample()[: c["feed"]])
            twin.step_count += 1
        calls.log = [] if s < CALL_STEPS else None
        out["loss_bits"].append(bits(tr.step(batch)))
        if calls.log is not None:
            out["calls"].append(calls.log)
        calls.log = None
        if s + 1 == DECAY_AFTER:
            tr.decay_lr()
    tr.finish()
    out["state_sha256"] = digest_all((tr.table, tr.m, tr.v))
    calls.trainer = None
    return out


def record(c, calls: Calls) -> dict:
    """The record of case c.  Raises if two runs of the case differ in any bit or call."""
    first, second = _run(c, calls), _run(c, calls)
    if first != second:
        raise RuntimeError(f"{c['key']}: two runs differ: {first} / {second}")
    return first


class _Patches:
    """setattr with an undo, for the run from the command line."""
    def __init__(self):
        self.undo = []

    def setattr(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def restore(self):
        for obj, name, value in reversed(self.undo):
            setattr(obj, name, value)
        self.undo = []


def pack(recorded: dict) -> dict:
    """The file's form of {key: record}: every distinct call sequence once, under a name that the cases use."""
    names, cases_out = {}, {}
    for key in sorted(recorded):
        rec = dict(recorded[key])
        rec["calls"] = [names.setdefault(tuple(seq), f"s{len(names)}") for seq in rec["calls"]]
        cases_out[key] = rec
    return {"sequences": {name: list(seq) for seq, name in names.items()}, "cases": cases_out}


def unpack(packed: dict) -> dict:
    """{key: record} with the call sequences written out, as record() returns them."""
    return {key: dict(rec, calls=[packed["sequences"][name] for name in rec["calls"]]) for key, rec in packed["cases"].items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="short hash of the tree that runs; written into the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "trainer_path_bits.json"))
    args = ap.parse_args()
    recorded = {}
    patches = _Patches()
    try:
        calls = Calls(patches.setattr)
        for c in cases():
            recorded[c["key"]] = record(c, calls)
            print(c["key"], flush=True)
    finally:
        patches.restore()
    packed = pack(recorded)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = {"recorded_at_commit": args.commit,
            "what": "LightGCNTrainer and ShardedLightGCNTrainer (world 1) on the cases of tools/record_trainer_bits.py: four "
                    "steps, decay_lr() after the second.  fp32 bit patterns of each step's loss in hex; one SHA-256 over the "
                    "bytes of table, m and v after finish(); SHA-256 of sample() before the first step; for steps 1 and 2 the "
                    "laplace_amd.ops calls in order (name[adjacency](keyword arguments that are not None)), by sequence name."}
    with open(args.out, "w") as f:      # one line per sequence and per case
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "sequences": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in packed["sequences"].items()))
        f.write('\n },\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in packed["cases"].items()))
        f.write("\n }\n}\n")
    print(f"{len(recorded)} cases, {len(packed['sequences'])} call sequences -> {args.out}")
