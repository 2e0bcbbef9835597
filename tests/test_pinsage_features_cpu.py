"""No GPU: the item feature projector's C ABI (sizes, argument checks, workspace queries), ItemFeatures' validation, the
id-only model's unchanged state_dict, and the torch twin of the projector that the GPU tests compare against.

The twin restates the reference's LinearProjector (pinsage/layers.py:14-46, 90-118): one embedding table per integer column,
a Linear over the float columns, the item id as one more integer column, everything summed — here in the documented order
(id row, table rows in column order, dense @ W^T + b), in the dtype of its parameters."""
import ctypes
import os
import subprocess

import pytest
import torch as t
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ProjectorTwin(nn.Module):
    """Assigned to PinSAGERef.proj (get_repr only calls it).  Parameter names: weight (the id table, so its state_dict key
    under PinSAGERef is `proj.weight` as the id-only oracle's), tables.<c>, w, b."""

    def __init__(self, n_items, hidden, cardinalities=(), n_dense=0, use_id=True, categorical=None, dense=None):
        super().__init__()
        if use_id:
            self.weight = nn.Parameter(t.zeros(n_items + 1, hidden))
        self.use_id = use_id
        self.tables = nn.ParameterList([nn.Parameter(t.zeros(c + 1, hidden)) for c in cardinalities])
        if n_dense:
            self.w = nn.Parameter(t.zeros(hidden, n_dense))
            self.b = nn.Parameter(t.zeros(hidden))
        self.n_dense = n_dense
        self.categorical, self.dense = categorical, dense

    def terms(self, ids):
        out = [self.weight[ids]] if self.use_id else []
        out += [tab[self.categorical[ids, c]] for c, tab in enumerate(self.tables)]
        if self.n_dense:
            out.append(self.dense[ids].to(self.w.dtype) @ self.w.t() + self.b)
        return out

    def forward(self, ids):
        h = None
        for term in self.terms(ids):
            h = term if h is None else h + term
        return h


def twin_state_from_model(model):
    """PinSAGEModel.state_dict() under PinSAGERef's names (the twin sits at `proj`)."""
    out = {}
    for k, v in model.state_dict().items():
        if k.startswith("projector.tables."):
            k = "proj.tables." + k.rsplit(".", 1)[1]
        elif k == "projector.weight":
            k = "proj.w"
        elif k == "projector.bias":
            k = "proj.b"
        out[k] = v.detach().cpu().clone()
    return out


def test_twin_on_a_hand_written_example():
    """3 items, 2 columns (cardinalities 2 and 3), hidden 2, one dense column; every number written out."""
    cat = t.tensor([[0, 2], [1, 0], [1, 2]])
    dense = t.tensor([[1.0], [2.0], [-1.0]])
    tw = ProjectorTwin(3, 2, (2, 3), 1, True, cat, dense)
    with t.no_grad():
        tw.weight.copy_(t.tensor([[1., 2.], [3., 4.], [5., 6.], [99., 99.]]))
        tw.tables[0].copy_(t.tensor([[10., 20.], [30., 40.], [77., 77.]]))
        tw.tables[1].copy_(t.tensor([[100., 200.], [300., 400.], [500., 600.], [88., 88.]]))
        tw.w.copy_(t.tensor([[0.5], [-1.0]]))
        tw.b.copy_(t.tensor([0.25, 0.75]))
    got = tw(t.tensor([0, 1, 2, 1]))
    want = t.tensor([[1 + 10 + 500 + 0.75, 2 + 20 + 600 - 0.25],
                     [3 + 30 + 100 + 1.25, 4 + 40 + 200 - 1.25],
                     [5 + 30 + 500 - 0.25, 6 + 40 + 600 + 1.75],
                     [3 + 30 + 100 + 1.25, 4 + 40 + 200 - 1.25]])
    assert t.equal(got, want)
    no_id = ProjectorTwin(3, 2, (2, 3), 0, False, cat, None)
    with t.no_grad():
        no_id.tables[0].copy_(tw.tables[0]); no_id.tables[1].copy_(tw.tables[1])
    assert t.equal(no_id(t.tensor([2])), t.tensor([[530., 640.]]))
    # the padding rows (the last of every table) are never looked up
    got.sum().backward()
    assert float(tw.tables[0].grad[2].abs().sum()) == 0 and float(tw.tables[1].grad[3].abs().sum()) == 0
    assert t.equal(tw.tables[0].grad[1], t.tensor([3., 3.]))     # items 1, 2, 1


def test_segmented_sum_emulation_on_a_hand_written_example():
    """The association the GPU tests pin (tests/segsum_emulation.py), on values where the order shows: 2^24 + 1 rounds back
    to 2^24 in float32.  Key 5 comes first in the sorted list: 66 references = all of piece 0 and two of piece 1."""
    import numpy as np
    import segsum_emulation as E
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    keys = [9, 5, 9, 9] + [5] * 65
    vals = [big, big, one, one] + [one] * 65
    sums = E.segmented_sum(np.array(keys), np.array(vals, dtype=np.float32)[:, None])
    assert sorted(sums) == [5, 9]
    assert sums[9][0] == big               # ((0 + big) + 1) + 1 in list order (the stable sort keeps it); 1 + 1 first: big + 2
    assert sums[5][0] == big + np.float32(2.0)   # piece 0: big + 63 ones = big; piece 1: 1 + 1; one chain over all 66: big
    k, v = E.projector_references([np.array([0, 0, 1]), np.array([7, 8, 7])], np.arange(6, dtype=np.float32).reshape(3, 2))
    assert k.tolist() == [0, 0, 1, E.SLOT + 7, E.SLOT + 8, E.SLOT + 7] and v[:, 0].tolist() == [0, 2, 4, 0, 2, 4]
    k, v = E.text_references([(np.array([0, 3, 3]), np.array([4, 4, 6]))], np.array([1, 0, 0]), np.array([[3.0], [1.0], [6.0]]))
    assert k.tolist() == [4, 4, 6, 4, 4, 6] and v[:, 0].tolist() == [np.float32(1.0) / np.float32(3.0)] * 3 + [2.0] * 3


# ---- C ABI -------------------------------------------------------------------------------------------------------------
NEW = ["mi_pinsage_project_sizeof", "mi_pinsage_project_workspace_bytes", "mi_pinsage_project_f32",
       "mi_pinsage_project_bwd_workspace_bytes", "mi_pinsage_project_bwd_f32", "mi_pinsage_project_clear_f32", "mi_adam_multi_f32"]


def test_header_binding_and_library_agree_on_the_new_entries():
    from laplace_amd import _lib
    from test_abi import _declared
    declared = _declared()
    assert _lib.exported_symbols() == declared
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in declared and name in exported, name
    assert set(declared) <= exported
    assert _lib.MI_ABI_VERSION == 14 and _lib.lib().mi_abi_version() == 14
    assert "#define MI_ABI_VERSION 14" in open(os.path.join(ROOT, "include", "laplace_hip.h")).read()


def test_sizeof_self_check():
    from laplace_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.ItemProjector) == L.mi_pinsage_project_sizeof(0)
    assert ctypes.sizeof(_lib.ItemProjectorGrads) == L.mi_pinsage_project_sizeof(1)
    assert L.mi_pinsage_project_sizeof(2) == -1
    # existing descriptors keep their layout
    for which, cls in enumerate((_lib.PinsageModel, _lib.PinsageStepBatch, _lib.PinsageConv, _lib.PinsageStepBlock,
                                 _lib.PinsageGradList)):
        assert ctypes.sizeof(cls) == L.mi_pinsage_step_sizeof(which)


def _desc(hidden=16, n_cols=2, n_dense=4, n_items=100, use_id=True):
    """A descriptor whose pointers are aligned non-null addresses that are never dereferenced on the host."""
    from laplace_amd import _lib
    d = _lib.ItemProjector()
    d.hidden, d.n_cols, d.n_items = hidden, n_cols, n_items
    fake = 1 << 20
    d.x = fake
    for c in range(min(n_cols, _lib.MI_PROJECTOR_MAX_COLS)):
        d.tables[c], d.table_rows[c] = fake, 51
    d.id_table = fake if use_id else None
    d.n_dense, d.ld_dense = n_dense, max(n_dense, 1)
    if n_dense:
        d.dense = d.w = d.b = fake
    return d


def test_null_descriptors_are_bad_arguments():
    from laplace_amd import _lib
    L = _lib.lib()
    d, g = _desc(), _lib.ItemProjectorGrads()
    fake = 1 << 20
    assert L.mi_pinsage_project_f32(None, 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_bwd_f32(None, ctypes.byref(g), 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_bwd_f32(ctypes.byref(d), None, 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_clear_f32(None, ctypes.byref(g), 4, None, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_clear_f32(ctypes.byref(d), None, 4, None, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_adam_multi_f32(None, 3, 1e-3, 0.9, 0.999, 1e-8, 1, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_workspace_bytes(None, 4) == 0 and L.mi_pinsage_project_bwd_workspace_bytes(None, 4) == 0
    # a null output / gradient / table pointer, a negative n, nothing to project, n beyond the catalogue without ids
    assert L.mi_pinsage_project_f32(ctypes.byref(d), 4, None, None, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_f32(ctypes.byref(d), -1, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_f32(ctypes.byref(d), 101, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    assert L.mi_pinsage_project_f32(ctypes.byref(d), 4, None, fake, 18, None, 0, None) == _lib.MI_ERR_BAD_ARG      # ldo % 4
    assert L.mi_pinsage_project_bwd_f32(ctypes.byref(d), ctypes.byref(g), 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    empty = _desc(n_cols=0, n_dense=0, use_id=False)
    assert L.mi_pinsage_project_f32(ctypes.byref(empty), 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG
    no_table = _desc()
    no_table.tables[1] = None
    assert L.mi_pinsage_project_f32(ctypes.byref(no_table), 4, None, fake, 16, None, 0, None) == _lib.MI_ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(hidden=130), dict(hidden=6), dict(n_cols=17)], ids=["hidden130", "hidden6", "cols17"])
def test_unsupported_shapes_are_refused_before_any_launch(kw):
    """No GPU here: a launch would fail with a runtime error (> 0), so MI_ERR_UNSUPPORTED also shows nothing was enqueued."""
    from laplace_amd import _lib
    L = _lib.lib()
    d, g = _desc(**kw), _lib.ItemProjectorGrads()
    fake = 1 << 20
    ws = 1 << 30
    assert L.mi_pinsage_project_f32(ctypes.byref(d), 8, None, fake, 256, fake, ws, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_pinsage_project_f32(ctypes.byref(d), 8, fake, fake, 256, fake, ws, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_pinsage_project_bwd_f32(ctypes.byref(d), ctypes.byref(g), 8, None, fake, 256, fake, ws, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_pinsage_project_clear_f32(ctypes.byref(d), ctypes.byref(g), 8, None, None) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_pinsage_project_workspace_bytes(ctypes.byref(d), 8) == 0
    assert L.mi_pinsage_project_bwd_workspace_bytes(ctypes.byref(d), 8) == 0


def test_short_workspace_is_refused():
    from laplace_amd import _lib
    L = _lib.lib()
    d, g = _desc(), _lib.ItemProjectorGrads()
    fake = 1 << 20
    for c in range(2):
        g.g_tables[c] = fake
    g.g_id_table = g.g_w = g.g_b = fake
    need = L.mi_pinsage_project_bwd_workspace_bytes(ctypes.byref(d), 64)
    assert L.mi_pinsage_project_bwd_f32(ctypes.byref(d), ctypes.byref(g), 64, None, fake, 16, fake, need - 1, None) == _lib.MI_ERR_WORKSPACE


@pytest.mark.parametrize("kw", [dict(), dict(hidden=128, n_cols=16, n_dense=512), dict(hidden=4, n_cols=1, n_dense=0, use_id=False),
                                dict(hidden=64, n_cols=0, n_dense=5, use_id=False)])
def test_workspace_queries_are_positive_and_do_not_shrink(kw):
    from laplace_amd import _lib
    L = _lib.lib()
    d = _desc(n_items=1 << 20, **kw)
    for query in (L.mi_pinsage_project_workspace_bytes, L.mi_pinsage_project_bwd_workspace_bytes):
        last = 0
        for n in [0, 1, 2, 63, 64, 65, 100, 127, 128, 129, 500, 1000, 1023, 1024, 3000, 8191, 8192, 8193, 16384, 105542, 1 << 20]:
            got = query(ctypes.byref(d), n)
            assert got > 0 and got >= last, (query, n, got, last)
            last = got


# ---- ItemFeatures / PinSAGEModel ---------------------------------------------------------------------------------------
def test_item_features_validation():
    from laplace_amd.pinsage.model import ItemFeatures
    cat, dense = t.tensor([[0, 3], [2, 1], [1, 0]]), t.zeros(3, 2)
    f = ItemFeatures(cat, dense)
    assert f.cardinalities == (3, 4) and f.n_items == 3 and f.n_cols == 2 and f.n_dense == 2
    assert ItemFeatures(cat, cardinalities=(5, 4)).cardinalities == (5, 4)
    assert ItemFeatures(dense=dense).n_cols == 0
    with pytest.raises(ValueError):
        ItemFeatures()
    with pytest.raises(ValueError, match="int64"):
        ItemFeatures(cat.to(t.int32))
    with pytest.raises(ValueError, match="int64"):
        ItemFeatures(cat[:, 0])                                  # rank 1
    with pytest.raises(ValueError, match="float32"):
        ItemFeatures(cat, dense.double())
    with pytest.raises(ValueError, match="float32"):
        ItemFeatures(dense=dense[0])
    with pytest.raises(ValueError, match="items"):
        ItemFeatures(cat, t.zeros(4, 2))
    with pytest.raises(ValueError, match="negative"):
        ItemFeatures(t.tensor([[0, -1], [1, 0]]))
    with pytest.raises(ValueError, match="cardinality"):
        ItemFeatures(cat, cardinalities=(3, 3))                  # code 3 in column 1
    with pytest.raises(ValueError):
        ItemFeatures(cat, cardinalities=(3,))
    with pytest.raises(ValueError):
        ItemFeatures(t.zeros(3, 17, dtype=t.int64))


def test_id_only_model_is_unchanged_and_use_id_needs_features():
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel
    I, H, L = 20, 8, 2
    t.manual_seed(3)
    m = PinSAGEModel(I, H, L)
    want = ["bias", "proj.weight"] + [f"convs.{l}.{lin}.{wb}" for l in range(L) for lin in "QW" for wb in ("weight", "bias")]
    assert list(m.state_dict().keys()) == want
    assert [n for n, _ in m.named_parameters()] == want
    assert not m.featured
    # the same draws as the construction always made: Embedding, xavier over it, then the layers
    t.manual_seed(3)
    emb = nn.Embedding(I + 1, H)
    nn.init.xavier_uniform_(emb.weight)
    assert t.equal(m.proj.weight, emb.weight)
    t.manual_seed(3)
    again = PinSAGEModel(I, H, L, features=None, use_id=True)
    assert all(t.equal(a, b) for a, b in zip(m.state_dict().values(), again.state_dict().values()))
    with pytest.raises(ValueError):
        PinSAGEModel(I, H, L, features=None, use_id=False)
    f = ItemFeatures(t.randint(0, 5, (I, 3)), t.randn(I, 2), cardinalities=(5, 5, 7))
    with pytest.raises(ValueError):
        PinSAGEModel(I + 1, H, L, features=f)
    both = PinSAGEModel(I, H, L, features=f)
    assert [tuple(x.shape) for x in both.projector.tables] == [(6, H), (6, H), (8, H)]
    assert tuple(both.projector.weight.shape) == (H, 2) and float(both.projector.bias.abs().sum()) == 0
    assert list(both.state_dict().keys())[: len(want)] == want
    assert sum(1 for p in both.parameters()) == len(want) + 5          # the id table is registered once
    only = PinSAGEModel(I, H, L, features=f, use_id=False)
    assert not hasattr(only, "proj") and "proj.weight" not in only.state_dict() and tuple(only.bias.shape) == (I, 1)


def test_native_step_refuses_data_parallel_features():
    from laplace_amd.pinsage.model import ItemFeatures, PinSAGEModel
    from laplace_amd.pinsage.native import NativePinSAGEStep
    m = PinSAGEModel(8, 4, 1, features=ItemFeatures(t.randint(0, 3, (8, 1))))
    opt = t.optim.Adam(m.parameters())
    with pytest.raises(ValueError, match="data_parallel with item features"):
        NativePinSAGEStep(m, opt, data_parallel=True)
    assert "CUDA" in NativePinSAGEStep.unsupported_reason(m, opt)        # CPU parameters: declined, with the reason
