"""No GPU: the bag-of-words text term of the item feature projector — its torch twin (which the GPU tests compare against),
the C ABI of mi_pinsage_text_* (sizes, argument checks, workspace queries), TextColumn / ItemFeatures(text=...) validation,
TextColumn.from_strings, and the state_dict of models with and without text.

The twin restates the reference's BagOfWords (pinsage/layers.py:49-87: the sum of one embedding row per token divided by the
length) in the documented order: one chain in ascending position, one division, an empty bag contributing zero, the bags
added after ProjectorTwin's terms in column order; everything in the dtype of its parameters."""
import ctypes
import os
import subprocess

import pytest
import torch as t
from torch import nn

from test_pinsage_features_cpu import ProjectorTwin, twin_state_from_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TextTwin(ProjectorTwin):
    """ProjectorTwin plus the bags.  text: one (ptr int64 [n_items + 1], tok integer [>= 1]) CSR per column; parameter names
    as ProjectorTwin's, then text_tables.<c>."""

    def __init__(self, n_items, hidden, text, vocabs, **base):
        super().__init__(n_items, hidden, **base)
        self.text_tables = nn.ParameterList([nn.Parameter(t.zeros(v, hidden)) for v in vocabs])
        self.text = [(ptr.long(), tok.long()) for ptr, tok in text]

    def bag(self, c, ids):
        (ptr, tok), E = self.text[c], self.text_tables[c]
        p0 = ptr[ids]
        ln = ptr[ids + 1] - p0
        s = t.zeros(len(ids), E.shape[1], dtype=E.dtype)
        for p in range(int(ln.max()) if len(ids) else 0):
            x = E[tok[(p0 + p).clamp(max=tok.numel() - 1)]]
            s = t.where((p < ln)[:, None], x if p == 0 else s + x, s)
        return t.where((ln > 0)[:, None], s / ln.clamp(min=1).to(E.dtype)[:, None], t.zeros_like(s))

    def terms(self, ids):
        return super().terms(ids) + [self.bag(c, ids) for c in range(len(self.text_tables))]


def text_twin_state_from_model(model):
    """PinSAGEModel.state_dict() under PinSAGERef's names with a TextTwin at `proj`."""
    out = {}
    for k, v in twin_state_from_model(model).items():
        if k.startswith("projector.text_tables."):
            k = "proj.text_tables." + k.rsplit(".", 1)[1]
        out[k] = v
    return out


def _column(rows, vocab, L=None, pad=0):
    from laplace_amd.pinsage.model import TextColumn
    L = L or max(1, max(len(r) for r in rows))
    tokens = t.full((len(rows), L), pad, dtype=t.int64)
    for i, r in enumerate(rows):
        tokens[i, : len(r)] = t.tensor(r, dtype=t.int64)
    return TextColumn(tokens, t.tensor([len(r) for r in rows]), vocab, pad_id=pad)


def test_twin_on_a_hand_written_example():
    """3 items with bags [1, 2] / [] / [3, 1, 3], vocabulary 4, hidden 2; every number written out."""
    col = _column([[1, 2], [], [3, 1, 3]], 4)
    assert col.ptr.tolist() == [0, 2, 2, 5] and col.tok.tolist() == [1, 2, 3, 1, 3] and col.tok.dtype == t.int32
    assert (col.max_len, col.nnz, col.n_items) == (3, 5, 3)
    E = t.tensor([[100., 100.], [9., 12.], [5., 2.], [3., 6.]])
    tw = TextTwin(3, 2, [(col.ptr, col.tok)], [4], use_id=False)
    with t.no_grad():
        tw.text_tables[0].copy_(E)
    got = tw(t.tensor([0, 1, 2, 1]))
    assert t.equal(got, t.tensor([[(9 + 5) / 2, (12 + 2) / 2], [0., 0.], [(3 + 9 + 3) / 3, (6 + 12 + 6) / 3], [0., 0.]]))
    # after an id row: one chain, text last; the empty bag adds zero
    both = TextTwin(3, 2, [(col.ptr, col.tok)], [4], use_id=True)
    with t.no_grad():
        both.text_tables[0].copy_(E)
        both.weight.copy_(t.tensor([[1., 2.], [3., 4.], [5., 6.], [99., 99.]]))
    assert t.equal(both(t.tensor([2, 1])), t.tensor([[5. + 5., 6. + 8.], [3., 4.]]))
    # gradient: g / len per reference; the token used twice in item 2 counts twice; the unused token and pads get nothing
    tw64 = TextTwin(3, 2, [(col.ptr, col.tok)], [4], use_id=False).double()
    with t.no_grad():
        tw64.text_tables[0].copy_(E.double())
    g = t.tensor([[1., 10.], [7., 7.], [3., 30.]], dtype=t.float64)
    tw64(t.tensor([0, 1, 2])).backward(g)
    want = t.tensor([[0., 0.], [1 / 2 + 3 / 3, 10 / 2 + 30 / 3], [1 / 2, 10 / 2], [2 * 3 / 3, 2 * 30 / 3]], dtype=t.float64)
    assert t.allclose(tw64.text_tables[0].grad, want, rtol=0, atol=1e-15)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
NEW = ["mi_pinsage_text_sizeof", "mi_pinsage_text_f32", "mi_pinsage_text_bwd_workspace_bytes", "mi_pinsage_text_bwd_f32",
       "mi_pinsage_text_clear_f32"]
FAKE = 1 << 20


def test_header_binding_and_library_agree_on_the_text_entries():
    from laplace_amd import _lib
    from test_abi import _declared
    declared = _declared()
    assert _lib.exported_symbols() == declared
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in declared and name in exported and hasattr(_lib.lib(), name), name
    assert _lib.MI_ABI_VERSION == 14 and _lib.lib().mi_abi_version() == 14      # additive: the version stays
    header = open(os.path.join(ROOT, "include", "laplace_hip.h")).read()
    assert "#define MI_ABI_VERSION 14" in header and "#define MI_PROJECTOR_MAX_TEXT 4" in header
    assert _lib.MI_PROJECTOR_MAX_TEXT == 4


def test_sizeof_self_check():
    from laplace_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.TextColumns) == L.mi_pinsage_text_sizeof(0) == 16 + 4 * 4 * 8
    assert L.mi_pinsage_text_sizeof(1) == -1 and L.mi_pinsage_text_sizeof(-1) == -1
    # the existing descriptors keep their layout
    assert ctypes.sizeof(_lib.ItemProjector) == L.mi_pinsage_project_sizeof(0)
    assert ctypes.sizeof(_lib.ItemProjectorGrads) == L.mi_pinsage_project_sizeof(1)
    for which, cls in enumerate((_lib.PinsageModel, _lib.PinsageStepBatch, _lib.PinsageConv, _lib.PinsageStepBlock,
                                 _lib.PinsageGradList)):
        assert ctypes.sizeof(cls) == L.mi_pinsage_step_sizeof(which)


def _desc(width=16, n_text=2, n_items=100):
    """A descriptor whose pointers are aligned non-null addresses that are never dereferenced on the host."""
    from laplace_amd import _lib
    d = _lib.TextColumns()
    d.width, d.n_text, d.n_items = width, n_text, n_items
    for c in range(min(n_text, _lib.MI_PROJECTOR_MAX_TEXT)):
        d.ptr[c] = d.tok[c] = d.tables[c] = FAKE
        d.vocab[c] = 50
    return d


def _grads(n=4, value=FAKE):
    from laplace_amd import _lib
    g = _lib.TextGradTables()
    for c in range(n):
        g[c] = value
    return g


def test_null_and_misaligned_arguments_are_bad_arguments():
    from laplace_amd import _lib
    L, BAD = _lib.lib(), _lib.MI_ERR_BAD_ARG
    d, g = _desc(), _grads()
    ws = 1 << 30
    assert L.mi_pinsage_text_f32(None, 4, None, FAKE, 16, 0, None) == BAD
    assert L.mi_pinsage_text_bwd_f32(None, g, 4, None, FAKE, 16, 64, FAKE, ws, None) == BAD
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), None, 4, None, FAKE, 16, 64, FAKE, ws, None) == BAD
    assert L.mi_pinsage_text_clear_f32(None, g, 4, None, None) == BAD
    assert L.mi_pinsage_text_clear_f32(ctypes.byref(d), None, 4, None, None) == BAD
    assert L.mi_pinsage_text_bwd_workspace_bytes(None, 4, 64) == 0
    # the output: null, misaligned, too narrow, ldo % 4; accumulate outside {0, 1}
    for out, ldo, acc in ((None, 16, 0), (FAKE + 4, 16, 0), (FAKE, 12, 0), (FAKE, 18, 0), (FAKE, 16, 2)):
        assert L.mi_pinsage_text_f32(ctypes.byref(d), 4, None, out, ldo, acc, None) == BAD, (out, ldo, acc)
    # n < 0, n beyond the catalogue without ids
    assert L.mi_pinsage_text_f32(ctypes.byref(d), -1, None, FAKE, 16, 0, None) == BAD
    assert L.mi_pinsage_text_f32(ctypes.byref(d), 101, None, FAKE, 16, 0, None) == BAD
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, -1, None, FAKE, 16, 64, FAKE, ws, None) == BAD
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 101, None, FAKE, 16, 64, FAKE, ws, None) == BAD
    assert L.mi_pinsage_text_clear_f32(ctypes.byref(d), g, 101, None, None) == BAD
    # the gradient: null, misaligned, ldg % 4; a negative bound; a null / misaligned gradient table
    for gp, ldg, bound in ((None, 16, 64), (FAKE + 8, 16, 64), (FAKE, 18, 64), (FAKE, 16, -1)):
        assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 4, None, gp, ldg, bound, FAKE, ws, None) == BAD, (gp, ldg, bound)
    for bad_g in (_grads(1), _grads(4, FAKE + 4)):
        assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), bad_g, 4, None, FAKE, 16, 64, FAKE, ws, None) == BAD
        assert L.mi_pinsage_text_clear_f32(ctypes.byref(d), bad_g, 4, None, None) == BAD
    # the descriptor: no column, no items, a null / misaligned ptr, tok or table, an empty vocabulary
    for field, value in (("ptr", None), ("ptr", FAKE + 4), ("tok", None), ("tok", FAKE + 2), ("tables", None), ("tables", FAKE + 4),
                         ("vocab", 0)):
        bad = _desc()
        getattr(bad, field)[1] = value
        assert L.mi_pinsage_text_f32(ctypes.byref(bad), 4, None, FAKE, 16, 0, None) == BAD, (field, value)
        assert L.mi_pinsage_text_bwd_f32(ctypes.byref(bad), g, 4, None, FAKE, 16, 64, FAKE, ws, None) == BAD, (field, value)
        assert L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(bad), 4, 64) == 0
    for kw in (dict(n_text=0), dict(n_items=0)):
        assert L.mi_pinsage_text_f32(ctypes.byref(_desc(**kw)), 0, None, FAKE, 16, 0, None) == BAD, kw


@pytest.mark.parametrize("kw", [dict(width=6), dict(width=516), dict(width=0), dict(n_text=5)], ids=["width6", "width516", "width0", "text5"])
def test_unsupported_shapes_are_refused_before_any_launch(kw):
    """No GPU here: a launch would fail with a runtime error (> 0), so MI_ERR_UNSUPPORTED also shows nothing was enqueued."""
    from laplace_amd import _lib
    L = _lib.lib()
    d, g = _desc(**kw), _grads()
    ws = 1 << 30
    for ids in (None, FAKE):
        assert L.mi_pinsage_text_f32(ctypes.byref(d), 8, ids, FAKE, 1024, 0, None) == _lib.MI_ERR_UNSUPPORTED
        assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 8, ids, FAKE, 1024, 64, FAKE, ws, None) == _lib.MI_ERR_UNSUPPORTED
        assert L.mi_pinsage_text_clear_f32(ctypes.byref(d), g, 8, ids, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(d), 8, 64) == 0


def test_short_workspace_is_refused():
    from laplace_amd import _lib
    L = _lib.lib()
    d, g = _desc(), _grads()
    need = L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(d), 64, 700)
    assert need > 0
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 64, None, FAKE, 16, 700, FAKE, need - 1, None) == _lib.MI_ERR_WORKSPACE
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 64, None, FAKE, 16, 700, None, need, None) == _lib.MI_ERR_WORKSPACE
    # the workspace of a smaller bound does not serve a larger one
    small = L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(d), 64, 100)
    assert L.mi_pinsage_text_bwd_f32(ctypes.byref(d), g, 64, None, FAKE, 16, 100_000, FAKE, small, None) == _lib.MI_ERR_WORKSPACE


@pytest.mark.parametrize("kw", [dict(), dict(width=512, n_text=4), dict(width=4, n_text=1), dict(width=128, n_text=3)])
def test_workspace_query_is_positive_and_does_not_shrink(kw):
    from laplace_amd import _lib
    L = _lib.lib()
    d = _desc(n_items=1 << 20, **kw)
    ns = [0, 1, 2, 63, 64, 65, 100, 127, 128, 129, 500, 1000, 1023, 1024, 3000, 8191, 8192, 8193, 16384, 105542, 1 << 20]
    bounds = [0, 1, 63, 64, 65, 1000, 4095, 4096, 4097, 100_000, 1 << 20, 1 << 24]
    table = [[L.mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(d), n, b) for b in bounds] for n in ns]
    for i, row in enumerate(table):
        for j, got in enumerate(row):
            assert got > 0, (ns[i], bounds[j])
            assert i == 0 or got >= table[i - 1][j], (ns[i], bounds[j])
            assert j == 0 or got >= row[j - 1], (ns[i], bounds[j])


# ---- TextColumn / ItemFeatures / PinSAGEModel --------------------------------------------------------------------------
def test_text_column_validation():
    from laplace_amd.pinsage.model import TextColumn
    tokens, lengths = t.tensor([[3, 1, 9], [2, 9, 9], [9, 9, 9]]), t.tensor([2, 1, 0])
    col = TextColumn(tokens, lengths, 4, pad_id=9)              # the pad (9 >= vocab) is never read
    assert col.ptr.tolist() == [0, 2, 3, 3] and col.tok.tolist() == [3, 1, 2] and col.ptr.dtype == t.int64
    assert (col.n_items, col.vocab_size, col.max_len, col.nnz, col.pad_id) == (3, 4, 2, 3, 9)
    empty = TextColumn(tokens, t.zeros(3, dtype=t.int64), 4)
    assert empty.ptr.tolist() == [0, 0, 0, 0] and empty.nnz == 0 and empty.tok.numel() == 1 and empty.max_len == 0
    with pytest.raises(ValueError, match="int64"):
        TextColumn(tokens.to(t.int32), lengths, 4)
    with pytest.raises(ValueError, match="int64"):
        TextColumn(tokens[0], lengths, 4)                       # rank 1
    with pytest.raises(ValueError, match="int64"):
        TextColumn(tokens, lengths.to(t.int32), 4)
    with pytest.raises(ValueError, match="int64"):
        TextColumn(tokens, lengths[:, None], 4)
    with pytest.raises(ValueError, match="items"):
        TextColumn(tokens, lengths[:2], 4)
    with pytest.raises(ValueError, match="length"):
        TextColumn(tokens, t.tensor([2, 4, 0]), 4)              # beyond L
    with pytest.raises(ValueError, match="length"):
        TextColumn(tokens, t.tensor([2, -1, 0]), 4)
    with pytest.raises(ValueError, match="token"):
        TextColumn(tokens, lengths, 3)                          # token 3 in item 0's bag
    with pytest.raises(ValueError, match="token"):
        TextColumn(t.tensor([[-1, 0]]), t.tensor([1]), 3)
    with pytest.raises(ValueError, match="token"):
        TextColumn(tokens, t.tensor([3, 1, 0]), 4)              # the third position of item 0 holds the pad
    with pytest.raises(ValueError):
        TextColumn(tokens, lengths, 0)


def test_item_features_with_text():
    from laplace_amd.pinsage.model import ItemFeatures
    cat, dense = t.tensor([[0, 3], [2, 1], [1, 0]]), t.zeros(3, 2)
    col = _column([[1], [], [2, 2]], 3)
    only = ItemFeatures(text=[col])                              # text alone is a feature set
    assert (only.n_items, only.n_cols, only.n_dense, only.n_text) == (3, 0, 0, 1) and only.cardinalities == ()
    every = ItemFeatures(cat, dense, text=(col, col))
    assert (every.n_items, every.n_cols, every.n_dense, every.n_text) == (3, 2, 2, 2) and every.cardinalities == (3, 4)
    assert ItemFeatures(cat).n_text == 0 and ItemFeatures(cat).text == ()
    with pytest.raises(TypeError):
        ItemFeatures(cat, dense, None, [col])                    # keyword-only
    with pytest.raises(ValueError):
        ItemFeatures(text=[])                                    # still nothing
    with pytest.raises(ValueError):
        ItemFeatures(text=[col] * 5)
    with pytest.raises(ValueError):
        ItemFeatures(text=[t.zeros(3, 2, dtype=t.int64)])        # not a TextColumn
    with pytest.raises(ValueError, match="items"):
        ItemFeatures(cat, text=[_column([[1], []], 3)])
    with pytest.raises(ValueError, match="items"):
        ItemFeatures(text=[col, _column([[1], []], 3)])
    with pytest.raises(ValueError):
        ItemFeatures(text=[col], cardinalities=(3,))
    with pytest.raises(ValueError, match="P % 4"):
        only.with_pooled_text(col, t.zeros(3, 6))
    with pytest.raises(ValueError, match="P % 4"):
        only.with_pooled_text(col, t.zeros(3, 516))
    with pytest.raises(ValueError, match="float32"):
        only.with_pooled_text(col, t.zeros(3, 8, dtype=t.float64))
    with pytest.raises(ValueError, match="float32"):
        only.with_pooled_text(col, t.zeros(4, 8))                # rows != vocab_size


def test_from_strings_on_five_sentences():
    from laplace_amd.pinsage.model import TextColumn
    texts = ["Blue cotton shirt", "blue  SHIRT\tblue", "", "Wool hat", "red cotton   hat "]
    col, itos = TextColumn.from_strings(texts)
    # by frequency, ties alphabetically: blue 3, cotton 2, hat 2, shirt 2, red 1, wool 1
    assert itos == ["<unk>", "<pad>", "blue", "cotton", "hat", "shirt", "red", "wool"]
    assert col.vocab_size == 8 and col.n_items == 5 and col.pad_id == 1
    assert col.ptr.tolist() == [0, 3, 6, 6, 8, 11]
    assert col.tok.tolist() == [2, 3, 5, 2, 5, 2, 7, 4, 6, 3, 4]
    rare, itos2 = TextColumn.from_strings(texts, min_freq=2)
    assert itos2 == ["<unk>", "<pad>", "blue", "cotton", "hat", "shirt"]
    assert rare.tok.tolist() == [2, 3, 5, 2, 5, 2, 0, 4, 0, 3, 4] and rare.ptr.tolist() == col.ptr.tolist()


def test_models_with_and_without_text_share_keys_and_draws():
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel, WeightedSAGEConv
    I, H, L = 20, 8, 2
    g = t.Generator().manual_seed(1)
    cat, dense = t.randint(0, 5, (I, 2), generator=g), t.randn(I, 3, generator=g)
    cols = [_column([[int(x) for x in t.randint(0, 11, (int(n),), generator=g)] for n in t.randint(0, 4, (I,), generator=g)], 11)
            for _ in range(2)]
    base = ["bias", "proj.weight"] + [f"convs.{l}.{lin}.{wb}" for l in range(L) for lin in "QW" for wb in ("weight", "bias")]
    plain_keys = base + ["projector.weight", "projector.bias", "projector.tables.0", "projector.tables.1"]
    t.manual_seed(3)
    plain = PinSAGEModel(I, H, L, features=ItemFeatures(cat, dense, cardinalities=(5, 5)))
    assert list(plain.state_dict().keys()) == plain_keys and [n for n, _ in plain.named_parameters()] == plain_keys
    # the draws a model without text always made: the id table, the layers, the tables, the Linear
    t.manual_seed(3)
    emb = nn.Embedding(I + 1, H)
    nn.init.xavier_uniform_(emb.weight)
    convs = [WeightedSAGEConv(H, H, H) for _ in range(L)]
    tabs = [nn.init.xavier_uniform_(t.empty(6, H)) for _ in range(2)]
    w = nn.init.xavier_uniform_(t.empty(H, 3))
    assert t.equal(plain.proj.weight, emb.weight) and t.equal(plain.projector.weight, w)
    assert all(t.equal(a, b) for a, b in zip(plain.projector.tables, tabs))
    assert all(t.equal(a.Q.weight, b.Q.weight) and t.equal(a.W.weight, b.W.weight) for a, b in zip(plain.convs, convs))
    # with text: the non-text keys first and unchanged, the same draws for them, the text tables drawn last
    t.manual_seed(3)
    texted = PinSAGEModel(I, H, L, features=ItemFeatures(cat, dense, cardinalities=(5, 5), text=cols))
    keys = list(texted.state_dict().keys())
    assert keys[: len(plain_keys)] == plain_keys and keys[len(plain_keys):] == ["projector.text_tables.0", "projector.text_tables.1"]
    assert all(t.equal(texted.state_dict()[k], plain.state_dict()[k]) for k in plain_keys)
    assert [tuple(x.shape) for x in texted.projector.text_tables] == [(11, H), (11, H)]
    bound = (6.0 / (11 + H)) ** 0.5
    assert all(0 < float(x.abs().max()) <= bound for x in texted.projector.text_tables)      # xavier-uniform
    pl = texted.projector.parameter_list()
    assert pl[0] is texted.proj.weight and pl[-2] is texted.projector.text_tables[0] and pl[-1] is texted.projector.text_tables[1]
    assert pl[3] is texted.projector.weight and pl[4] is texted.projector.bias and len(pl) == 7
    assert sum(1 for _ in texted.parameters()) == len(plain_keys) + 2
    # text alone: no id table, no other projector parameter
    only = PinSAGEModel(I, H, L, features=ItemFeatures(text=cols[:1]), use_id=False)
    assert list(only.state_dict().keys()) == ["bias"] + base[2:] + ["projector.text_tables.0"]
    assert not only.projector.has_base and texted.projector.has_base
    # the twin's names cover the model's
    names = text_twin_state_from_model(texted)
    assert "proj.text_tables.1" in names and "proj.tables.0" in names and "proj.w" in names and "proj.weight" in names


def test_native_step_accepts_text_models_up_to_the_device_check():
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    m = PinSAGEModel(3, 4, 1, features=ItemFeatures(text=[_column([[1], [], [2, 2]], 3)]), use_id=False)
    opt = t.optim.Adam(m.parameters())
    assert "CUDA" in NativePinSAGEStep.unsupported_reason(m, opt)        # CPU parameters: the only objection
    with pytest.raises(ValueError, match="data_parallel with item features"):
        NativePinSAGEStep(m, opt, data_parallel=True)
