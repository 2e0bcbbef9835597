"""PinSAGE evaluation (N5) without a GPU: latest-item selection on host CSRs, hits@K on host tensors, and the argument checks
of mi_pinsage_embed_items_f32 (they return before anything touches a device)."""
import ctypes

import numpy as np
import pytest
import torch as t


def test_latest_item_is_the_last_entry_of_the_row():
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.graph_io import _adj_dict
    from laplace_amd.pinsage.evaluation import LatestNNRecommender
    users = AdjList({0: [5, 3, 9], 1: [2], 2: [7, 1]}, 3)
    assert LatestNNRecommender().latest_items(users).tolist() == [9, 2, 1]
    # a transaction log (time order) -> rows in time order -> the latest purchase is the last entry
    u = np.array([1, 0, 1, 2, 0, 1])
    a = np.array([4, 8, 6, 3, 2, 0])
    rows = AdjList(_adj_dict(u, a), 3)
    assert LatestNNRecommender().latest_items(rows).tolist() == [2, 0, 3]
    ptr, idx = t.tensor([0, 2, 3]), t.tensor([1, 4, 0])
    assert LatestNNRecommender().latest_items((ptr, idx)).tolist() == [4, 0]


def test_a_user_without_interactions_raises():
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.evaluation import LatestNNRecommender
    with pytest.raises(ValueError):
        LatestNNRecommender().latest_items(AdjList({0: [1], 2: [3]}, 3))
    with pytest.raises(TypeError):
        LatestNNRecommender().latest_items(object())
    with pytest.raises(ValueError):
        LatestNNRecommender().recommend(AdjList({0: [1]}, 1), 0, None, t.zeros(4, 4))


def test_prec_on_host_tensors():
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.pinsage.evaluation import prec
    held = AdjList({0: [3], 1: [5, 6], 3: [0]}, 4)          # user 2: nothing held out
    rec = t.tensor([[1, 3], [6, -1], [0, 1], [-1, -1]])
    assert prec(rec, held) == 0.5                          # users 0 and 1 hit; 2 has nothing, 3 only pads
    assert prec(t.tensor([[3, 0], [7, 8], [5, 6], [0, 0]]), held) == 0.5
    with pytest.raises(ValueError):
        prec(rec[:3], held)
    assert prec(rec, (t.zeros(5, dtype=t.long), t.zeros(0, dtype=t.long))) == 0.0


def test_embed_entry_rejects_shapes_outside_the_kernel():
    from laplace_amd import _lib
    L = _lib.lib()
    d = _lib.PinsageModel()
    d.n_layers, d.hidden, d.n_items, d.proj = 2, 16, 100, 4096
    for l in range(2):
        c = d.conv[l]
        c.q_w, c.q_b, c.w_w, c.w_b = 4096, 4096, 4096, 4096
    fake = 4096

    def call(T=3, walks=10, restart=0.5, ws_bytes=1 << 30):
        return L.mi_pinsage_embed_items_f32(ctypes.byref(d), fake, fake, fake, fake, 2, restart, walks, T, 1, 0, fake, fake,
                                            ws_bytes, None)

    assert L.mi_pinsage_embed_items_f32(None, fake, fake, fake, fake, 2, 0.5, 10, 3, 1, 0, fake, fake, 1 << 30, None) == -1
    assert call(restart=1.0) == -1
    assert call(T=17) == _lib.MI_ERR_UNSUPPORTED
    assert call(walks=1000) == _lib.MI_ERR_UNSUPPORTED          # the walks of a seed do not fit a block
    assert call(ws_bytes=16) == _lib.MI_ERR_WORKSPACE
    for layers, hidden in ((5, 16), (0, 16), (2, 6), (2, 132)):
        d.n_layers, d.hidden = layers, hidden
        assert call() == _lib.MI_ERR_UNSUPPORTED, (layers, hidden)
    need = L.mi_pinsage_embed_items_workspace_bytes(105_542, 16, 3)
    assert need >= 2 * 105_542 * 3 * 8 + 3 * 105_542 * 16 * 4
