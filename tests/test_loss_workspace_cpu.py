"""CPU: the workspace needs of the three loss entries, mi_rank_loss_workspace_bytes, mi_bpr_workspace_bytes and
mi_inbatch_softmax_workspace_bytes, are what they were before the entries shared the buffers of csrc/refsum.hpp.  The
functions are host-only (tests/asan_driver.py loads the library without a device); the values below were printed by the
build of commit 46a864b, the last one where train.hip and inbatch.hip each sized their own buffers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asan_driver import L  # noqa: E402

RANK = {(1, 1): 1054720, (1, 4): 1054720, (1, 16): 1054720, (64, 1): 1065472, (64, 4): 1081856, (64, 16): 1147904,
        (300, 1): 1132544, (300, 4): 1209600, (300, 16): 1517824, (16384, 1): 5341184, (16384, 4): 9568256,
        (16384, 16): 26476544}                                      # (batch, M)
INBATCH = {(1, 4): 1052672, (1, 128): 1054464, (1, 256): 1057536, (64, 4): 1057024, (64, 128): 1185536, (64, 256): 1318656,
           (300, 4): 1087744, (300, 128): 1692416, (300, 256): 2317056, (16384, 4): 3096576, (16384, 128): 36110336,
           (16384, 256): 70189056}                                  # (batch, d), group 32


def test_rank_and_bpr_workspace_bytes_are_as_before():
    for (batch, m), want in RANK.items():
        assert int(L.mi_rank_loss_workspace_bytes(batch, m)) == want, (batch, m)
        if m == 1:
            assert int(L.mi_bpr_workspace_bytes(batch)) == want, batch


def test_inbatch_workspace_bytes_are_as_before():
    for (batch, d), want in INBATCH.items():
        for group in (32, 1024):                                    # the group does not enter the size
            assert int(L.mi_inbatch_softmax_workspace_bytes(batch, d, group)) == want, (batch, d, group)
    assert int(L.mi_inbatch_softmax_workspace_bytes(64, 260, 32)) == 0 and int(L.mi_inbatch_softmax_workspace_bytes(64, 32, 48)) == 0
