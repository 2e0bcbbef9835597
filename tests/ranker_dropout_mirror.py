"""The native ranker executor's Philox feature dropout, restated in numpy (csrc/exec_common.hpp: dropout_segment, which
dropout_kernel, dropout_pair_kernel and ranker_prep_dropout_kernel share; csrc/norm.hip: gather_cat_dropout_kernel draws the same).

    float4 index i of the dropped matrix (row-major, so i = flat element index // 4)
    draw   = Philox4x32-10(counter = (i & 0xffffffff, i >> 32, site, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32))
    thr    = (uint32) min(4294967040.f, p * 4294967296.f)          evaluated in float32, truncated
    keep element 4 i + j  where  draw[j] >= thr;  kept elements are multiplied by  1.f / (1.f - p)  (float32)

Sites: 2 l + t for the input of encoder layer l and node type t (0 = customer, 1 = article); 64 + j for the input of decoder
layer j.  The decoder's first dropout is drawn by the gather itself (site 64, the flat float4 index of the [n_label, 2 C]
matrix) — the same counters as a dropout launch over that matrix.  The backward regenerates every mask from these counters.

Importable without a GPU; tests/test_ranker_step_cases_cpu.py holds it against hand-computed draws.
"""
import numpy as np

from oracle.philox import philox4x32


def threshold(p: float) -> int:
    """The kernel's `thr`: float32 arithmetic, clamped below 2^32, truncated towards zero."""
    prod = np.float32(p) * np.float32(4294967296.0)
    return int(min(np.float32(4294967040.0), prod))


def scale(p: float) -> np.float32:
    """The kernel's `1.0f / (1.0f - p)`."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(n_elements: int, p: float, seed: int, step: int, site: int) -> np.ndarray:
    """bool[n_elements]: which elements of a matrix of n_elements floats (a multiple of 4) the dropout at `site` keeps."""
    assert n_elements % 4 == 0 and n_elements >= 0
    i = np.arange(n_elements // 4, dtype=np.uint64)
    draws = philox4x32(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), site, step & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                       (seed >> 32) & 0xFFFFFFFF)
    draws = np.stack([np.asarray(d, dtype=np.uint64) for d in draws], axis=1).reshape(-1)     # element 4 i + j <- draw[j]
    return draws >= np.uint64(threshold(p))


def multiplier(shape, p: float, seed: int, step: int, site: int) -> np.ndarray:
    """float64[shape]: 0 where the element is dropped, the kernel's float32 scale where it is kept."""
    n = int(np.prod(shape))
    return np.where(keep_mask(n, p, seed, step, site), np.float64(scale(p)), 0.0).reshape(shape)


def encoder_site(layer: int, node_type: int) -> int:
    return 2 * layer + node_type


def decoder_site(layer: int) -> int:
    return 64 + layer
