"""GPU: the bag-of-words text term of PinSAGE's item feature projector (mi_pinsage_text_f32 / _bwd_f32 / _clear_f32) against
the torch twin of tests/test_pinsage_text_cpu.py, the model's autograd and native iterations with text against PinSAGERef +
twin on the mirror's batches, the catalogue pass with text, the one-time pooling of pretrained vectors, and what the text is
for: items without interactions placed by their words."""
import copy

import numpy as np
import pytest
import torch as t

from oracle import pinsage_ref as PR
from test_pinsage_text_cpu import TextTwin, text_twin_state_from_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
LENGTHS = (0, 1, 2, 7, 64, 65)


def _text(n_items, vocabs, seed, lengths=LENGTHS):
    """One TextColumn (on the CPU) per vocabulary: every length drawn from `lengths`, tokens uniform over the vocabulary; the
    padding holds vocab (out of range: it must never be read)."""
    from laplace_amd.pinsage.model import TextColumn
    g = t.Generator().manual_seed(seed)
    cols = []
    for v in vocabs:
        ln = t.tensor(lengths)[t.randint(0, len(lengths), (n_items,), generator=g)]
        L = max(1, int(max(lengths)))
        tokens = t.randint(0, v, (n_items, L), generator=g)
        tokens[t.arange(L)[None, :] >= ln[:, None]] = v
        cols.append(TextColumn(tokens, ln, v, pad_id=v))
    return cols


def _features(n_items, cards, n_dense, text, seed):
    from laplace_amd.pinsage.model import ItemFeatures
    g = t.Generator().manual_seed(seed)
    cat = t.stack([t.randint(0, c, (n_items,), generator=g) for c in cards], 1).to(DEV) if cards else None
    dense = t.randn(n_items, n_dense, generator=g).to(DEV) if n_dense else None
    return ItemFeatures(cat, dense, cardinalities=cards if cards else None, text=[c.to(DEV) for c in text])


def _twin_of(model, dtype=t.float32):
    """The CPU twin holding the model's projector weights, features and text in `dtype`."""
    pr = model.projector
    text = [(getattr(pr, f"text_ptr_{c}").cpu(), getattr(pr, f"text_tok_{c}").cpu()) for c in range(pr.n_text)]
    tw = TextTwin(model.n_items, model.hidden, text, pr.text_vocab, cardinalities=pr.cardinalities,
                  n_dense=0 if pr.weight is None else pr.weight.shape[1], use_id=pr.id_weight is not None,
                  categorical=None if pr.x is None else pr.x.cpu(), dense=None if pr.dense is None else pr.dense.cpu())
    with t.no_grad():
        if tw.use_id:
            tw.weight.copy_(pr.id_weight.cpu())
        for a, b in zip(tw.tables, pr.tables):
            a.copy_(b.cpu())
        if tw.n_dense:
            tw.w.copy_(pr.weight.cpu()); tw.b.copy_(pr.bias.cpu())
        for a, b in zip(tw.text_tables, getattr(pr, "text_tables", [])):
            a.copy_(b.cpu())
    return tw.to(dtype)


def _references(tw, c, rows):
    """(row index, token, length of the row's bag) of every reference of column c over `rows`, in (row, position) order."""
    ptr, tok = tw.text[c]
    ln = ptr[rows + 1] - ptr[rows]
    rep = t.repeat_interleave(t.arange(len(rows)), ln)
    start = t.cumsum(ln, 0) - ln
    pos = ptr[rows][rep] + (t.arange(int(ln.sum())) - start[rep])
    return rep, tok[pos], ln[rep]


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------
FWD_CASES = [(4, 1, (), 0, False), (16, 2, (50, 7), 0, True), (128, 4, (132, 3, 30), 5, True)]


@pytest.mark.parametrize("vocab", [50, 5000])
@pytest.mark.parametrize("hidden,T,cards,F,use_id", FWD_CASES, ids=["h4t1", "h16t2id2cat", "h128t4id3cat5f"])
def test_forward_against_the_twin(hidden, T, cards, F, use_id, vocab):
    from laplace_amd.pinsage.model import PinSAGEModel
    I = 1000
    t.manual_seed(hidden + T)
    model = PinSAGEModel(I, hidden, 1, features=_features(I, cards, F, _text(I, (vocab,) * T, 7 + T), 3), use_id=use_id).to(DEV)
    pr = model.projector
    assert pr.has_base == bool(cards or F or use_id)
    if F:
        with t.no_grad():
            pr.bias.normal_(0, 0.1)
    tw32, tw64 = _twin_of(model), _twin_of(model, t.float64)
    tw_abs = copy.deepcopy(tw64)
    with t.no_grad():
        for tab in tw_abs.text_tables:
            tab.abs_()
    C = len(cards)
    g = t.Generator().manual_seed(5)
    for n in (0, 1, 63, 1000):
        for ids in (t.randint(0, I, (n,), generator=g) // 3 * 3 % I if n else t.zeros(0, dtype=t.int64), None):
            rows = t.arange(n) if ids is None else ids
            with t.no_grad():
                got = pr.project(None, n=n) if ids is None else pr.project(ids.to(DEV))
                assert got.shape == (n, hidden)
                if ids is not None:
                    assert t.equal(pr(ids.to(DEV)), got)                  # the autograd Function's forward is the same call
                if n and F == 0:
                    assert t.equal(got.cpu(), tw32(rows)), (n, ids is None)  # the f32 chain in the documented order, bitwise
                if n:
                    terms = tw64.terms(rows)
                    want = sum(terms)
                    mag = sum(x.abs() for x in terms[: len(terms) - T]) + sum(tw_abs.bag(c, rows) for c in range(T))   # a bag's |rows| / len
                    if F:      # the dense term's own |products|
                        mag = mag - terms[-1 - T].abs() + tw64.dense[rows].double().abs() @ tw64.w.abs().t() + tw64.b.abs()
                    longest = max(int((tw64.text[c][0][rows + 1] - tw64.text[c][0][rows]).max()) for c in range(T))
                    err = (got.cpu().double() - want).abs()
                    bound = (F + C + T + longest + 3) * EPS * mag
                    assert bool((err <= bound).all()), (n, ids is None, float((err / bound.clamp(min=1e-300)).max()))


@pytest.mark.parametrize("P", [300, 512])
def test_pooled_pretrained_vectors_against_a_float64_mean(P):
    """BagOfWordsPretrained's frozen half: the forward kernel at width = P over the catalogue, appended to dense."""
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel
    I, V = 700, 900
    col = _text(I, (V,), 21)[0]
    g = t.Generator().manual_seed(P)
    vectors, dense = t.randn(V, P, generator=g), t.randn(I, 3, generator=g)
    feats = ItemFeatures(dense=dense.to(DEV)).with_pooled_text(col.to(DEV), vectors.to(DEV))
    assert feats.n_dense == 3 + P and feats.n_text == 0 and t.equal(feats.dense[:, :3].cpu(), dense)
    got = feats.dense[:, 3:].cpu().double()
    ptr, tok = col.ptr, col.tok.long()
    want, mag = t.zeros(I, P, dtype=t.float64), t.zeros(I, P, dtype=t.float64)
    item = t.repeat_interleave(t.arange(I), ptr[1:] - ptr[:-1])
    ln = (ptr[1:] - ptr[:-1]).clamp(min=1).double()[:, None]
    want.index_add_(0, item, vectors.double()[tok]); mag.index_add_(0, item, vectors.double().abs()[tok])
    want, mag = want / ln, mag / ln
    assert bool((got[(ptr[1:] == ptr[:-1])] == 0).all())                   # an empty bag pools to exactly zero
    bound = (col.max_len + 3) * EPS * mag
    assert bool(((got - want).abs() <= bound).all())
    only = ItemFeatures(text=[col.to(DEV)]).with_pooled_text(col.to(DEV), vectors.to(DEV))      # no dense before: the pooled alone
    assert only.n_dense == P and only.n_text == 1 and t.equal(only.dense, feats.dense[:, 3:])
    if P == 300:       # the Linear over [dense | pooled] trains like any dense feature
        m = PinSAGEModel(I, 16, 1, features=feats, use_id=False).to(DEV)
        assert tuple(m.projector.weight.shape) == (16, 303) and bool(t.isfinite(m.projector.project(None)).all())


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def _check_backward(I, hidden, vocabs, lengths, cards, use_id, n, seed, all_items=False, ids=None, text=None):
    from laplace_amd.pinsage.model import PinSAGEModel
    t.manual_seed(seed)
    text = _text(I, vocabs, seed + 2, lengths) if text is None else text
    model = PinSAGEModel(I, hidden, 1, features=_features(I, cards, 0, text, seed), use_id=use_id).to(DEV)
    pr = model.projector
    g = t.Generator().manual_seed(seed + 1)
    if ids is None and not all_items:
        ids = t.randint(0, max(I // 2, 1), (n,), generator=g)          # repeats: n draws from I / 2 ids
    rows = t.arange(n) if ids is None else ids
    gout = t.randn(n, hidden, generator=g)
    params = pr.parameter_list()
    T = len(vocabs)
    runs = []
    for _ in range(2):
        bufs = [t.full_like(p, SENTINEL) for p in params]
        pr.project_backward(None if ids is None else ids.to(DEV), gout.to(DEV), bufs)
        runs.append(bufs)
    bufs = runs[0]
    assert all(t.equal(a, b) for a, b in zip(*runs))                       # no atomics: equal bits
    tw = _twin_of(model, t.float64)
    if n:
        tw(rows).backward(gout.double())
    absg = gout.double().abs()
    longest_run = 0
    for c in range(T):
        got = bufs[len(bufs) - T + c].cpu().double()
        ref = tw.text_tables[c].grad if n else None
        r, tok, ln = _references(tw, c, rows)
        count = t.zeros(got.shape[0], dtype=t.float64).index_add_(0, tok, t.ones(len(tok), dtype=t.float64))
        sums = t.zeros_like(got).index_add_(0, tok, absg[r] / ln.double()[:, None])
        touched = count > 0
        assert bool((got[~touched] == SENTINEL).all()), c                    # rows nobody references: left as the caller had them
        if n and bool(touched.any()):
            bound = count[:, None] * EPS * sums        # per table row: (references of the row) * 2^-23 * sum |g / len| over the run
            err = (got - ref).abs()
            assert bool((err[touched] <= bound[touched]).all()), (c, float(err[touched].max()))
            longest_run = max(longest_run, int(count.max()))
    # the other parameters' gradients are the projector's own, as without text (the bound of its own test)
    names = (["weight"] if use_id else []) + [f"tables.{c}" for c in range(len(cards))]
    for name, buf in zip(names, bufs):
        codes = rows if name == "weight" else tw.categorical[rows, int(name.split(".")[1])]
        got = buf.cpu().double()
        count = t.zeros(got.shape[0], dtype=t.float64).index_add_(0, codes, t.ones(n, dtype=t.float64))
        assert bool((got[count == 0] == SENTINEL).all()), name
        if n:
            bound = count[:, None] * EPS * t.zeros_like(got).index_add_(0, codes, absg)
            err = (got - dict(tw.named_parameters())[name].grad).abs()
            assert bool((err[count > 0] <= bound[count > 0]).all()), name
    return model, longest_run


def test_backward_long_runs_against_float64_autograd():
    """vocab 2: two runs of about ten thousand references (hundreds of chunks each, combined in chunk order); 50: runs of about
    four hundred that cross chunk borders at every offset; 100 000: runs of one (and a few of two)."""
    _, longest = _check_backward(2500 * 2, 32, (2, 50, 100_000), tuple(range(13)), (7,), True, 3000, 11)
    assert longest >= 8000


def test_backward_one_item_of_65_equal_tokens_crosses_exactly_one_border():
    from laplace_amd.pinsage.model import TextColumn
    tokens = t.full((3, 65), 1, dtype=t.int64)
    tokens[1, :] = 2
    col = TextColumn(tokens, t.tensor([65, 3, 0]), 4)
    _, longest = _check_backward(3, 16, (4,), None, (), False, 1, 19, ids=t.tensor([0]), text=[col])
    assert longest == 65


@pytest.mark.parametrize("case", ["n150h16", "n150h20", "one_item_of_65_equal_tokens"])
def test_backward_bits_are_the_documented_association(case):
    """torch.equal with tests/segsum_emulation.py on every table row; rows nobody references keep the sentinel.  n = 150 rows
    over vocabularies (2, 50) with lengths 0 .. 5: the two tokens of the first column are runs over several pieces of 64, some
    bags are empty, and the bound passed (n x the longest bags) exceeds the actual count, so the sort sees padding keys."""
    import segsum_emulation as E
    from laplace_amd.pinsage.model import PinSAGEModel, TextColumn
    if case == "one_item_of_65_equal_tokens":
        I, hidden, ids = 3, 16, t.tensor([0])
        tokens = t.full((3, 65), 1, dtype=t.int64)
        tokens[1, :] = 2
        text = [TextColumn(tokens, t.tensor([65, 3, 0]), 4)]
    else:
        I, hidden = 300, int(case[-2:])
        ids = t.randint(0, I // 2, (150,), generator=t.Generator().manual_seed(29))
        text = _text(I, (2, 50), 31, tuple(range(6)))
    t.manual_seed(hidden)
    model = PinSAGEModel(I, hidden, 1, features=_features(I, (), 0, text, 5), use_id=False).to(DEV)
    pr = model.projector
    gout = t.randn(len(ids), hidden, generator=t.Generator().manual_seed(37))
    bufs = [t.full_like(p, SENTINEL) for p in pr.parameter_list()]
    pr.project_backward(ids.to(DEV), gout.to(DEV), bufs)
    columns = [(getattr(pr, f"text_ptr_{c}").cpu().numpy(), getattr(pr, f"text_tok_{c}").cpu().numpy()) for c in range(pr.n_text)]
    keys, values = E.text_references(columns, ids.numpy(), gout.numpy())
    if case != "one_item_of_65_equal_tokens":
        lens = [ptr[ids.numpy() + 1] - ptr[ids.numpy()] for ptr, _ in columns]
        assert len(keys) < pr.text_ref_bound(len(ids), True) and any((ln == 0).any() for ln in lens)
        assert (keys == 0).sum() > 2 * E.PIECE and (keys == 1).sum() > 2 * E.PIECE
    sums = E.segmented_sum(keys, values)
    for c, buf in enumerate(bufs):
        want = t.from_numpy(E.expected_tables(sums, c, buf, SENTINEL))
        assert t.equal(buf.cpu(), want), (c, float((buf.cpu() - want).abs().max()))


@pytest.mark.parametrize("case", ["n0", "all_empty", "n1"])
def test_backward_small(case):
    from laplace_amd.pinsage.model import TextColumn
    tokens = t.randint(0, 9, (40, 5), generator=t.Generator().manual_seed(2))
    ln = t.arange(40) % 6
    ln[::2] = 0                                                            # the even items have no text
    cols = [TextColumn(tokens, ln, 9), TextColumn(tokens.flip(1), ln.flip(0).clamp(max=5) * (t.arange(40) % 2), 9)]
    ids = {"n0": t.zeros(0, dtype=t.int64), "all_empty": t.tensor([0, 2, 2, 38, 10]), "n1": t.tensor([7])}[case]
    _, longest = _check_backward(40, 16, (9, 9), None, (3, 5), True, len(ids), 23, ids=ids, text=cols)
    assert (longest == 0) == (case != "n1")


def test_backward_whole_catalogue_without_ids():
    _check_backward(700, 128, (50, 5000), LENGTHS, (5,), True, 700, 17, all_items=True)


def test_clear_returns_the_buffers_to_all_zero():
    from laplace_amd.pinsage.model import PinSAGEModel
    I, H = 600, 32
    t.manual_seed(1)
    model = PinSAGEModel(I, H, 1, features=_features(I, (9,), 0, _text(I, (50, 3000), 4), 5)).to(DEV)
    pr = model.projector
    g = t.Generator().manual_seed(2)
    for ids in (t.randint(0, I, (500,), generator=g).to(DEV), None):
        n = I if ids is None else 500
        bufs = [t.zeros_like(p) for p in pr.parameter_list()]
        pr.project_backward(ids, t.randn(n, H, generator=g).to(DEV), bufs)
        assert all(float(b.abs().max()) > 0 for b in bufs)
        pr.clear_rows(ids, bufs)
        assert all(float(b.abs().max()) == 0.0 and not bool(t.signbit(b).any()) for b in bufs)


# ---- 3. the model's two iterations against PinSAGERef + twin ---------------------------------------------------------------------
_GRAPH = {}


def _shared_graph():
    if not _GRAPH:
        from test_gpu_pinsage_features import _pin_graph
        _GRAPH["g"] = _pin_graph(5, 2500, 800, 40000)
    return _GRAPH["g"]


@pytest.mark.parametrize("kind", ["id+cat+text", "text"])
@pytest.mark.parametrize("hidden,layers,walk", [(16, 2, 2), (64, 2, 3)])
def test_text_iterations_against_the_oracle_twin(hidden, layers, walk, kind):
    from laplace_amd.pinsage.model import PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I, SEED, B = 2500, 800, 31, 48
    users, items = _shared_graph()
    ucsr, icsr = PR.Csr(users.ptr, users.idx), PR.Csr(items.ptr, items.idx)
    smp = PinSAGESampler(users, items, U, I, batch_size=B, random_walk_length=walk, num_layers=layers, seed=SEED)
    t.manual_seed(hidden + layers)
    use_id = kind != "text"
    text = _text(I, (60, 500), 13, tuple(range(9)))
    model = PinSAGEModel(I, hidden, layers, features=_features(I, (7, 132) if use_id else (), 0, text, 9), use_id=use_id).to(DEV)
    with t.no_grad():
        model.bias.normal_(0, 0.1)
    for cv in model.convs:
        cv.dropout.p = 0.0
    ref = PR.PinSAGERef(I, hidden, layers)
    ref.proj = _twin_of(model)
    for cv in ref.convs:
        cv.dropout.p = 0.0
    lr = 3e-3
    opt, opt_ref = t.optim.Adam(model.parameters(), lr=lr), t.optim.Adam(ref.parameters(), lr=lr)
    assert NativePinSAGEStep.unsupported_reason(model, opt) is None
    probe, full = NativePinSAGEStep(model, opt, keep_grads=True), None
    model.train(); ref.train()
    to_ref = {k: k2 for k, k2 in zip(model.state_dict().keys(), text_twin_state_from_model(model).keys())}
    ref_params = dict(ref.named_parameters())
    assert sorted(to_ref.values()) == sorted(ref_params)
    table_params = [p for p in model.projector.parameter_list()]           # no Linear here: every one is a table

    def compare_grads(what, step, grads_ref):
        for n, p in model.named_parameters():
            g = grads_ref[to_ref[n]]
            scale = float(g.abs().max()) + 1e-12
            assert float((p.grad.cpu() - g).abs().max()) <= 2e-4 * scale + 1e-8, (what, step, n)

    for step in range(3):
        ref.load_state_dict(text_twin_state_from_model(model))
        got = smp.sample_batch(step)
        wh, wt, wn = PR.item_pairs(B, I, icsr, ucsr, SEED, step)
        want = PR.sample_from_item_pairs(wh, wt, wn, icsr, ucsr, layers, walk, 0.5, 10, 3, SEED, step)
        assert np.array_equal(got["seeds"].cpu().numpy(), want["seeds"])   # mirror batches are bit-equal
        opt_ref.zero_grad()
        lb = ref(t.from_numpy(want["seeds"]), tuple(t.from_numpy(x) for x in want["pos"]),
                 tuple(t.from_numpy(x) for x in want["neg"]), PR.to_torch_blocks(want["blocks"])).mean()
        lb.backward()
        grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
        # (a) the autograd path
        opt.zero_grad(set_to_none=True)
        la = model(got["seeds"], got["pos"], got["neg"], got["blocks"]).mean()
        la.backward()
        assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), ("autograd", step)
        compare_grads("autograd", step, grads_ref)
        for p in model.parameters():
            p.grad.zero_()
        # (b) the executor, gradients only
        la = probe.step(got)
        assert la is not None, probe.declined
        assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), ("native", step)
        compare_grads("native", step, grads_ref)
        for p in model.parameters():
            p.grad.zero_()                                                 # what the probe left behind
        # (c) the full iteration from the same weights
        before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        if full is None:
            full = NativePinSAGEStep(model, opt)
        assert full.step(got) is not None, full.declined
        opt_ref.step()
        for n, p in model.named_parameters():
            q, g, b = ref_params[to_ref[n]], grads_ref[to_ref[n]], before[n]
            big = g.abs() > 1e-3 * (float(g.abs().max()) + 1e-12) + 1e-7
            assert bool(big.any()), n
            assert t.allclose((p.detach().cpu() - b)[big], (q.detach() - b)[big], rtol=5e-2, atol=2e-6), (step, n)
            assert t.equal(p.detach().cpu()[g == 0], b[g == 0]) or step > 0   # rows never touched do not move on the first step
            assert float(opt.state[p]["step"]) == step + 1 == float(opt_ref.state[q]["step"])
        # the table gradients (the text tables' among them) and the scorer bias's are all-zero again
        for p in [model.bias] + table_params:
            assert float(p.grad.abs().max()) == 0.0


# ---- 4. catalogue pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["id+cat+text", "text"])
def test_catalogue_pass_with_text(kind):
    from laplace_amd.pinsage.model import PinSAGEModel, train_epoch
    from laplace_amd.pinsage.native import embed_items
    from laplace_amd.pinsage.sampler import PinSAGESampler
    from test_gpu_pinsage_eval import _graph
    U, I = 1500, 700
    users, items = _graph(7, U, 600, I, 20000)
    smp = PinSAGESampler(users, items, U, I, batch_size=32, random_walk_length=2, num_layers=2, seed=11)
    t.manual_seed(0)
    use_id = kind != "text"
    feats = _features(I, (7, 132) if use_id else (), 0, _text(I, (60, 500), 3, tuple(range(9))), 4)
    model = PinSAGEModel(I, 16, 2, features=feats, use_id=use_id).to(DEV)
    opt = t.optim.Adam(model.parameters(), lr=3e-3)
    losses = train_epoch(model, opt, smp, 10)
    assert len(losses) == 10 and all(np.isfinite(losses))
    step = smp.step
    with t.no_grad():
        assert embed_items(model, smp, step) is not None
    h = model.item_representations(smp)
    assert h.shape == (I, 16) and model.training
    model.eval()
    with t.no_grad():
        ref = model.batched_item_representations(smp, step, 97)
    model.train()
    assert float((h - ref).abs().max()) <= 1e-5
    assert t.equal(model.item_representations(smp, step=5), model.item_representations(smp, step=5))


# ---- 5. cold items --------------------------------------------------------------------------------------------------------------------
def test_cold_items_are_placed_by_their_text():
    """The recipe of test_cold_items_are_placed_by_their_features (600 users, 400 items, 12 000 edges, 8 planted communities with
    mix 0.85, the same 40 cold items, hidden 32, 300 iterations, lr 3e-3) with the item text in place of the community column:
    vocabulary 128 (0 = pad), community c owns the words 1 + 4c .. 4 + 4c, lengths uniform in 1 .. 12, each token from the own
    band with probability 0.75 and else uniform over 1 .. 127.  Score: the share of a cold item's 10 nearest warm items that lie
    in its community; chance = 1/8.  The CPU twin of this recipe measured 0.12 (id only), 0.945 (text only), 0.885 (id + text)."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel, TextColumn, train_epoch
    from laplace_amd.pinsage.sampler import PinSAGESampler
    U, I, K, V, LMAX = 600, 400, 8, 128, 12
    spec = S.SyntheticSpec(U, I, 12000, seed=3, communities=K, community_mix=0.85)
    ei = S.generate(spec)
    community = S.item_community(spec)
    rng = np.random.default_rng(1)
    np.stack([rng.integers(0, c, size=I) for c in (132, 30, 50)], 1)         # that test's column draws: the same cold items after them
    cold = rng.choice(I, 40, replace=False)
    lengths = rng.integers(1, LMAX + 1, size=I)
    own = rng.random((I, LMAX)) < 0.75
    tokens = np.where(own, 1 + 4 * community[:, None] + rng.integers(0, 4, size=(I, LMAX)), rng.integers(1, V, size=(I, LMAX)))
    tokens[np.arange(LMAX)[None, :] >= lengths[:, None]] = 0
    is_cold = np.zeros(I, dtype=bool)
    is_cold[cold] = True
    u, a = ei[0].numpy(), ei[1].numpy()
    keep = ~is_cold[a]
    users, items = AdjList.from_edges(u[keep], a[keep], U), AdjList.from_edges(a[keep], u[keep], I)
    assert all(items.ptr[i + 1] == items.ptr[i] for i in cold)
    col = TextColumn(t.from_numpy(tokens.astype(np.int64)), t.from_numpy(lengths.astype(np.int64)), V, pad_id=0)
    feats = ItemFeatures(text=[col.to(DEV)])
    warm = t.from_numpy(np.flatnonzero(~is_cold)).to(DEV)
    comm = t.from_numpy(community.astype(np.int64)).to(DEV)
    cold_t = t.from_numpy(np.sort(cold)).to(DEV)
    score = {}
    for kind, kw in (("id", dict()), ("text", dict(features=feats, use_id=False)), ("id+text", dict(features=feats))):
        t.manual_seed(0)
        model = PinSAGEModel(I, 32, 2, **kw).to(DEV)
        smp = PinSAGESampler(users, items, U, I, batch_size=32, random_walk_length=2, num_random_walks=10, num_neighbors=3,
                             num_layers=2, seed=5)
        opt = t.optim.Adam(model.parameters(), lr=3e-3)
        train_epoch(model, opt, smp, 300)
        h = model.item_representations(smp)
        near = (h[cold_t] @ h[warm].t()).topk(10, dim=1).indices
        score[kind] = float((comm[warm][near] == comm[cold_t][:, None]).float().mean())
    chance = 1.0 / K
    print(f"cold items, same-community share of the 10 nearest warm items: id {score['id']:.3f}, "
          f"text {score['text']:.3f}, id+text {score['id+text']:.3f} (chance {chance:.3f})")
    assert score["id"] <= 2 * chance
    assert score["text"] >= 4 * chance and score["text"] > score["id"]
    assert score["id+text"] >= 4 * chance and score["id+text"] > score["id"]
