"""Record the bits of the ranker's training iteration on each of its host paths (autograd, ranker_step.FusedRankerStep,
ranker_native.NativeRankerStep) and of ranker_native.NativeRankerForward into tests/golden/ranker_path_bits.json.

For every case and each of three consecutive iterations: the raw fp32 bits of the loss, and three SHA-256 digests: over the
bytes of every parameter's gradient, over both BatchNorm layers' running_mean / running_var / num_batches_tracked, and over
every parameter after the update (each digest walks all its tensors in named_parameters() order, so none is left out and the
file stays small); for inference the SHA-256 of the logits.  The committed file was recorded at the commit it names, the last one at
which each path wrote its stages out for itself; tests/test_gpu_ranker.py recomputes every case and compares for equality.  The
test takes its cases and its records from cases() and record() below, so the file and the test cannot drift apart.
    python3 tools/record_ranker_bits.py --commit <short hash of the tree that runs> [--out tests/golden/ranker_path_bits.json]"""
import argparse
import copy
import hashlib
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the model and graph of the tests (_hetero_setup)
import torch as t
from laplace_amd.utils.constants import Constants

DEV = "cuda"
ITERATIONS = 3
NORMS = ("encoder_layer_norm_customer", "encoder_layer_norm_article")
# (conv aggregation, categorical features through the embedding tables?); the dense feature widths are 6 and 4: pad and slice
ENCODER_FORMS = (("add", True), ("mean", True), ("max", False), ("add", False))


def bits(x) -> str:
    """The fp32 value's bit pattern, 8 hex digits."""
    return f"{t.as_tensor(x, dtype=t.float32).reshape(-1)[:1].cpu().view(t.int32).item() & 0xFFFFFFFF:08x}"


def digest(x) -> str:
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digest_all(named) -> str:
    """One SHA-256 over the bytes of every tensor of `named` (pairs of name and tensor) in their order, each behind its name."""
    h = hashlib.sha256()
    for name, x in named:
        h.update(name.encode())
        h.update(x.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def snapshot(model, loss) -> dict:
    """What one finished iteration left behind: the loss, every parameter's gradient, both BatchNorm layers' buffers and
    every parameter after the update."""
    return {"loss_bits": bits(loss),
            "grads_sha256": digest_all((n, p.grad) for n, p in model.named_parameters()),
            "norms_sha256": digest_all((f"{bn}.{k}", getattr(getattr(model, bn), k)) for bn in NORMS
                                       for k in ("running_mean", "running_var", "num_batches_tracked")),
            "params_sha256": digest_all(model.named_parameters())}


def batch_digest(x, ei, eli, y) -> str:
    """The inputs of an iteration: a difference here is the loader's or the sampler's, not the ranker's."""
    h = hashlib.sha256()
    for d in (x, ei):
        for k in d:
            h.update(digest(d[k]).encode())
    h.update(digest(eli).encode())
    h.update(digest(y).encode())
    return h.hexdigest()


def cases():
    out = []
    for path in ("autograd", "fused"):
        out += [dict(kind=path, aggr=a, embedding=e, key=f"{path}_{a}_{'embedding' if e else 'dense'}") for a, e in ENCODER_FORMS]
    out += [dict(kind="native", aggr=a, p_drop=p, labels=lab, key=f"native_{a}_drop{p}_{lab}")
            for a in ("add", "mean") for p in (0.0, 0.3) for lab in ("int64", "float32")]
    out += [dict(kind="sampler", stripped=s, key="sampler_batch" + ("_stripped" if s else "")) for s in (False, True)]
    out += [dict(kind="no_edges", key="no_edges"), dict(kind="no_label_edges", key="no_label_edges"),
            dict(kind="workspace", key="workspace_growth")]
    return out


def _loader_batches(loader):
    from laplace_amd.utils.get_info import select_properties
    for i, batch in enumerate(loader):
        if i == ITERATIONS:
            break
        yield select_properties(batch.to(DEV))


def _op_by_op(c):
    """Three iterations of training.py:19-34 through autograd, or through FusedRankerStep."""
    from laplace_amd.ranker_step import FusedRankerStep
    from test_gpu_ranker import _hetero_setup
    model, loader, _ = _hetero_setup(seed=11, aggr=c["aggr"], embedding=c["embedding"])
    opt = t.optim.Adam(model.parameters(), lr=0.01)
    fused = FusedRankerStep(model, opt) if c["kind"] == "fused" else None
    crit = t.nn.BCEWithLogitsLoss()
    model.train()
    out = []
    for x, ei, eli, y in _loader_batches(loader):
        if fused is not None:
            loss = fused.step({k: v.clone() for k, v in x.items()}, ei, eli, y)
            assert loss is not None
        else:
            opt.zero_grad()
            loss = crit(model({k: v.clone() for k, v in x.items()}, ei, eli).view(-1), y)
            loss.backward()
            opt.step()
        out.append(dict(snapshot(model, loss), batch_sha256=batch_digest(x, ei, eli, y)))
    return {"iterations": out}


def _native(c):
    from laplace_amd.ranker_native import NativeRankerStep
    from test_gpu_ranker import _hetero_setup
    model, loader, _ = _hetero_setup(seed=12, aggr=c["aggr"], embedding=True, p_drop=c["p_drop"])
    native = NativeRankerStep(model, t.optim.Adam(model.parameters(), lr=0.01), seed=1234)
    model.train()
    out = []
    for x, ei, eli, y in _loader_batches(loader):
        labels = y.long() if c["labels"] == "int64" else y.float()
        loss = native.step({k: v.clone() for k, v in x.items()}, ei, eli, labels)
        assert loss is not None, native.declined
        out.append(dict(snapshot(model, loss), batch_sha256=batch_digest(x, ei, eli, labels), iteration=native.iteration))
    return {"iterations": out}


def _sampler_setup():
    """The graph, sampler and model of test_native_ranker_step_with_the_device_sampler_and_training_loop."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.device_sampler import DeviceGraphSampler
    from laplace_amd.model.encoder_decoder import Encoder_Decoder_Model
    from laplace_amd.model.layers import get_SAGEConv_layers, get_linear_layers
    from laplace_amd.utils.get_info import get_feature_info
    spec = S.SyntheticSpec(3000, 500, 40_000, seed=4, deg_min=2, deg_max=200)
    graph, users, articles = S.generate_hetero(spec, customer_cards=(300, 2, 84, 4, 5, 2), article_cards=(100, 132, 30, 50))
    cfg = SimpleNamespace(k=12, num_neighbors=16, n_hop_neighbors=2, positive_edges_ratio=0.5, negative_edges_ratio=3.0, batch_size=24)
    sampler = DeviceGraphSampler(cfg, graph, users, articles, device=DEV, seed=0)
    first = sampler.sample(t.arange(24), step=0)
    t.manual_seed(0)
    model = Encoder_Decoder_Model(get_SAGEConv_layers(2, 128, 64, "add"), get_linear_layers(2, 128, 128, 1), get_feature_info(graph),
                                  first.metadata(), True, "sum", True, 0.0, 0.3).to(DEV)
    model.initialize_encoder_input_size(first)
    return sampler, model


def _twin(model):
    twin = copy.deepcopy(model)
    twin.embedding_layers = model.embedding_layers   # frozen tables, shared
    return twin


def _sampler(c):
    """One device-sampler batch through the native step, the fused step and the native forward: with the sampler's two
    attributes on its edge indices (`_sorted_csr`, `_reverse_of`: no sort anywhere), and with both stripped (two sorts in the
    native paths, four in the encoder)."""
    from laplace_amd.ranker_native import NativeRankerForward, NativeRankerStep
    from laplace_amd.ranker_step import FusedRankerStep
    sampler, model = _sampler_setup()
    batch = sampler.sample(t.arange(24, 48), step=1)
    x, ei = batch.x_dict, batch.edge_index_dict
    labelled = batch[Constants.edge_key]
    eli, y = labelled.edge_label_index, labelled.edge_label
    if c["stripped"]:
        ei = {k: v.clone() for k, v in ei.items()}
    has = {"__".join(k): [hasattr(v, "_sorted_csr"), hasattr(v, "_reverse_of")] for k, v in ei.items()}
    assert any(any(v) for v in has.values()) != c["stripped"]
    twin = _twin(model)
    native = NativeRankerStep(model, t.optim.Adam(model.parameters(), lr=0.01), seed=1234)
    fused = FusedRankerStep(twin, t.optim.Adam(twin.parameters(), lr=0.01))
    model.train(); twin.train()
    out = {"attributes": has, "batch_sha256": batch_digest(x, ei, eli, y), "native": [], "fused": []}
    t.manual_seed(77)                                  # the fused step's dropout masks are torch's
    for _ in range(ITERATIONS):
        loss = native.step(dict(x), ei, eli, y)
        assert loss is not None, native.declined
        out["native"].append(dict(snapshot(model, loss), iteration=native.iteration))
        loss = fused.step(dict(x), ei, eli, y.float())
        assert loss is not None
        out["fused"].append(snapshot(twin, loss))
    model.eval()
    forward = NativeRankerForward(model)
    logits = forward.logits(dict(x), ei, eli)
    assert logits is not None, forward.declined
    out["logits_sha256"] = digest(logits)
    return out


def _outcome(call, model, declined=lambda: None):
    """What a path does with a batch: its iteration's record, None with its decline string, or the exception's type."""
    try:
        got = call()
    except Exception as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):   # a device fault is no outcome to record
            raise
        return {"raises": type(e).__name__}
    if got is None:
        return {"returns": None, "declined": declined()}
    return snapshot(model, got) if got.numel() == 1 and model is not None else {"shape": list(got.shape), "sha256": digest(got)}


def _no_edges(c):
    """A hand-built batch whose buys relation (and its reverse) has no edge."""
    from laplace_amd.ranker_native import NativeRankerForward, NativeRankerStep
    from laplace_amd.ranker_step import FusedRankerStep
    from test_gpu_ranker import _hetero_setup
    model, loader, _ = _hetero_setup(seed=13, aggr="add", embedding=True)
    x, ei, eli, y = next(_loader_batches(loader))
    ei = {k: t.empty(2, 0, dtype=t.int64, device=DEV) for k in ei}
    m_fused, m_native = _twin(model), _twin(model)
    fused = FusedRankerStep(m_fused, t.optim.Adam(m_fused.parameters(), lr=0.01))
    native = NativeRankerStep(m_native, t.optim.Adam(m_native.parameters(), lr=0.01), seed=1234)
    m_fused.train(); m_native.train(); model.eval()
    forward = NativeRankerForward(model)
    fresh = lambda: {k: v.clone() for k, v in x.items()}
    return {"fused": _outcome(lambda: fused.step(fresh(), ei, eli, y), m_fused),
            "native": _outcome(lambda: native.step(fresh(), ei, eli, y), m_native, lambda: native.declined),
            "forward": _outcome(lambda: forward.logits(fresh(), ei, eli), None, lambda: forward.declined)}


def _no_label_edges(c):
    from laplace_amd.ranker_native import NativeRankerForward
    from test_gpu_ranker import _hetero_setup
    model, loader, _ = _hetero_setup(seed=13, aggr="add", embedding=True)
    x, ei, eli, _ = next(_loader_batches(loader))
    model.eval()
    got = NativeRankerForward(model).logits({k: v.clone() for k, v in x.items()}, ei, eli[:, :0])
    return {"shape": list(got.shape), "dtype": str(got.dtype), "sha256": digest(got)}


def _workspace(c):
    """The workspace growth rule: a batch, one larger in all four counts (customers, articles, edges, label edges), a
    smaller one."""
    from laplace_amd.ranker_native import NativeRankerStep
    sampler, model = _sampler_setup()
    native = NativeRankerStep(model, t.optim.Adam(model.parameters(), lr=0.01), seed=1234)
    model.train()
    out = []
    for step, n_users in enumerate((8, 24, 4)):
        batch = sampler.sample(t.arange(n_users), step=step + 1)
        labelled = batch[Constants.edge_key]
        loss = native.step(batch.x_dict, batch.edge_index_dict, labelled.edge_label_index, labelled.edge_label)
        assert loss is not None, native.declined
        counts = [int(batch[Constants.node_user].x.shape[0]), int(batch[Constants.node_item].x.shape[0]),
                  int(labelled.edge_index.shape[1]), int(labelled.edge_label.numel())]
        out.append({"counts": counts, "workspace_numel": int(native._ws.numel()), "loss_bits": bits(loss)})
    assert all(a < b for a, b in zip(out[0]["counts"], out[1]["counts"])), "the second batch must be larger in all four counts"
    assert all(a < b for a, b in zip(out[2]["counts"], out[1]["counts"])), "the third batch must be smaller"
    return {"steps": out}


_RECORD = {"autograd": _op_by_op, "fused": _op_by_op, "native": _native, "sampler": _sampler, "no_edges": _no_edges,
           "no_label_edges": _no_label_edges, "workspace": _workspace}


def record(c) -> dict:
    return _RECORD[c["kind"]](c)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="short hash of the tree that runs; written into the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ranker_path_bits.json"))
    args = ap.parse_args()
    recorded = {}
    for c in cases():
        recorded[c["key"]] = record(c)
        print(c["key"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = {"recorded_at_commit": args.commit,
            "what": "The ranker's iteration on its three host paths and NativeRankerForward, on the cases of "
                    "tools/record_ranker_bits.py: fp32 bit patterns of the loss in hex; one SHA-256 each over the bytes "
                    "of all gradients, all BatchNorm buffers and all updated parameters (name, then bytes, in "
                    "named_parameters() order); SHA-256 of the logits; workspace sizes in bytes."}
    with open(args.out, "w") as f:      # one line per case
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(recorded[k], sort_keys=True)}" for k in sorted(recorded)))
        f.write("\n }\n}\n")
    print(f"{len(recorded)} cases -> {args.out}")
