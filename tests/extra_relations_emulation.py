"""NumPy mirror of the attribute-relation rule (Config.other_edge_types; include/laplace_hip.h N1b, data/relations.py),
and the small graph the CPU and the GPU tests share.

Input: a collated batch's sorted article ids per sample (`article_ids` global ids, `article_ptr` int64[B + 1]) and a
relation as a CSR over the articles (rows strictly ascending).  Per sample s with articles a_0 < ... < a_{m-1}:
T nodes = the sorted distinct ids of the union of rel[a_j]; edges, for j ascending and e in rel[a_j] ascending,
(article_ptr[s] + j, T_ptr[s] + rank_s(e)).  Besides the edge list the two CSRs sorted by (row, column)."""
from types import SimpleNamespace

import numpy as np
import torch as t

ARTICLE, CUSTOMER = "article", "customer"
REL_A = (ARTICLE, "has_color", "colour_group_code")
REL_B = (ARTICLE, "has_tag", "tag")
U, A, N_TA, N_TB = 40, 30, 5, 70
ISLAND_USERS, ISLAND_ARTICLES = (37, 38, 39), (27, 28, 29)   # a component whose articles have no relation-B target
# relation B: rows of 0, 1 and 3 targets; ids on both sides of the 32-bit word borders (31 | 32, 63 | 64)
ROWS_B = {0: [31, 32, 63], 1: [64], 2: [0, 32, 69], 3: [31], 5: [63, 64, 65], 7: [5], 10: [32], 11: [33, 34, 35], 13: [64],
          17: [1, 31, 64], 20: [32], 24: [68]}


def emulate(article_ids, article_ptr, rel_ptr, rel_idx):
    article_ids, article_ptr = np.asarray(article_ids, dtype=np.int64), np.asarray(article_ptr, dtype=np.int64)
    rel_ptr, rel_idx = np.asarray(rel_ptr, dtype=np.int64), np.asarray(rel_idx, dtype=np.int64)
    B = article_ptr.shape[0] - 1
    t_ids, t_ptr, src, dst = [], [0], [], []
    for s in range(B):
        arts = article_ids[article_ptr[s]:article_ptr[s + 1]]
        assert (np.diff(arts) > 0).all()
        rows = [rel_idx[rel_ptr[a]:rel_ptr[a + 1]] for a in arts]
        flat = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
        mine = np.unique(flat)
        for j, row in enumerate(rows):
            assert (np.diff(row) > 0).all()
            src += [article_ptr[s] + j] * len(row)
            dst += list(t_ptr[-1] + np.searchsorted(mine, row))
        t_ids.append(mine)
        t_ptr.append(t_ptr[-1] + len(mine))
    t_ids = np.concatenate(t_ids) if t_ids else np.empty(0, dtype=np.int64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    na, nt = int(article_ptr[-1]), int(t_ptr[-1])

    def csr(rows, cols, n):
        order = np.lexsort((cols, rows))
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
        return ptr.astype(np.int32), cols[order].astype(np.int32)

    return {"T_ids": t_ids, "T_ptr": np.asarray(t_ptr, dtype=np.int64), "edge_index": np.stack([src, dst]).reshape(2, -1),
            "by_article": csr(src, dst, na), "by_target": csr(dst, src, nt)}


def set_restatement(article_ids, article_ptr, rel):
    """The rule once more, with sets: rel = {article: iterable of target ids}.  ([T ids per sample], [edges per sample],
    edges with sample-local indices)."""
    nodes, edges = [], []
    for s in range(len(article_ptr) - 1):
        arts = [int(a) for a in article_ids[article_ptr[s]:article_ptr[s + 1]]]
        T = sorted(set().union(*[set(rel.get(a, ())) for a in arts]))
        nodes.append(T)
        edges.append([(j, T.index(e)) for j, a in enumerate(arts) for e in sorted(set(rel.get(a, ())))])
    return nodes, edges


def rel_csr(rows: dict, n_articles: int):
    ptr = np.zeros(n_articles + 1, dtype=np.int64)
    for a in range(n_articles):
        ptr[a + 1] = ptr[a] + len(set(rows.get(a, ())))
    idx = np.asarray([e for a in range(n_articles) for e in sorted(set(rows.get(a, ())))], dtype=np.int64)
    return ptr, idx


def rows_a():
    return {a: [a % N_TA] for a in range(A)}      # every article exactly one target (the colour group of an H&M article)


def make_graph(relations=("A", "B"), empty_b=False, seed=0):
    """(graph, users AdjList, articles AdjList, config, {relation key: {article: targets}}): 40 users, 30 articles, about 150
    edges; users 37..39 buy only articles 27..29.  Relation A: 5 targets, one per article.  Relation B: 70 targets, ROWS_B (or
    no edge at all with empty_b).  The edge lists are shuffled and carry duplicates."""
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.hetero import HeteroData
    rng = np.random.default_rng(seed)
    us, as_ = [], []
    for u in range(U):
        if u in ISLAND_USERS:
            mine = rng.choice(ISLAND_ARTICLES, size=2, replace=False)
        else:
            mine = rng.choice(ISLAND_ARTICLES[0], size=int(rng.integers(2, 6)), replace=False)
        us += [u] * len(mine)
        as_ += [int(a) for a in mine]
    us, as_ = np.asarray(us, dtype=np.int64), np.asarray(as_, dtype=np.int64)
    g = HeteroData()
    g[CUSTOMER].x = t.from_numpy(rng.integers(0, 7, size=(U, 3)))
    g[ARTICLE].x = t.from_numpy(rng.integers(0, 9, size=(A, 2)))
    g[(CUSTOMER, "buys", ARTICLE)].edge_index = t.from_numpy(np.stack([us, as_]))
    rels, node_types, keys = {}, [CUSTOMER, ARTICLE], []
    for which in relations:
        key, n_t, rows = (REL_A, N_TA, rows_a()) if which == "A" else (REL_B, N_TB, {} if empty_b else ROWS_B)
        pairs = [(a, e) for a, row in rows.items() for e in row]
        pairs = pairs + pairs[:3]                                   # duplicates: dropped by the loader
        order = rng.permutation(len(pairs))
        ei = np.asarray([pairs[i] for i in order], dtype=np.int64).reshape(-1, 2).T
        g[key[2]].x = t.from_numpy(rng.integers(0, 4, size=(n_t, 2)))
        g[key].edge_index = t.from_numpy(np.ascontiguousarray(ei))
        rels[key] = rows
        node_types.append(key[2])
        keys.append(key)
    cfg = SimpleNamespace(k=4, num_neighbors=4, n_hop_neighbors=2, positive_edges_ratio=0.5, negative_edges_ratio=3.0,
                          batch_size=3, other_edge_types=keys, node_types=node_types)
    return g, AdjList.from_edges(us, as_, U), AdjList.from_edges(as_, us, A), cfg, rels


class IslandMatcher:
    """Evaluation-mode candidates: island users are proposed island articles only, the others a few of the rest."""

    def get_matches(self, u: int):
        if u in ISLAND_USERS:
            return np.asarray(ISLAND_ARTICLES, dtype=np.int64)
        return np.asarray([(u * 7 + i * 3) % ISLAND_ARTICLES[0] for i in range(4)], dtype=np.int64)
