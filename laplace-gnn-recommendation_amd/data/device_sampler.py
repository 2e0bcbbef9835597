"""On-device N-hop sampler: whole batches of the ranker's training subgraphs are
sampled, relabelled and collated on the GPU (csrc/sampler.hip) — the mini-batch never exists on
the host.  Same algorithm as `GraphDataset.__getitem__` (data/dataset.py of the reference) + the
PyG collate; draws come from a counter-based Philox stream (oracle/sampler_ref.py mirrors it)."""
from __future__ import annotations

import ctypes
import os
import math
from typing import Iterator, Optional

import numpy as np
import torch as t
from torch import Tensor

from .. import _lib
from .._lib import SamplerDesc, SamplerRelation, SamplerRelationOut, check
from ..hetero import HeteroData
from ..utils.constants import Constants
from .dataset import AdjList
from .relations import resolve_relations


def candidate_csr(matchers, num_users: int):
    """(ptr int64[U + 1], idx int64[]) of cat(m.get_matches(u) for m in matchers) per user.  Matchers that can
    answer for all users at once (`matches_for_all`) are not looped over."""
    dense = [m.matches_for_all(num_users) if hasattr(m, "matches_for_all") else None for m in matchers]
    if matchers and all(d is not None for d in dense):  # all vectorised: concatenate per user, drop the -1 pads
        cat = np.concatenate([np.asarray(d, dtype=np.int64) for d in dense], axis=1)
        keep = cat >= 0
        ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
        return ptr, cat[keep]
    per_user_counts = np.zeros(num_users, dtype=np.int64)
    blocks = []
    for m, d in zip(matchers, dense):
        if d is not None:  # [U, k] int64, -1 = no proposal
            d = np.asarray(d, dtype=np.int64)
            keep = d >= 0
            blocks.append((np.repeat(np.arange(num_users), d.shape[1])[keep.reshape(-1)], d[keep]))
            per_user_counts += keep.sum(axis=1)
        else:
            us, its = [], []
            for u in range(num_users):
                got = np.asarray(m.get_matches(u)).astype(np.int64).reshape(-1)
                us.append(np.full(got.shape[0], u, dtype=np.int64))
                its.append(got)
                per_user_counts[u] += got.shape[0]
            blocks.append((np.concatenate(us), np.concatenate(its)))
    users = np.concatenate([b[0] for b in blocks]) if blocks else np.empty(0, dtype=np.int64)
    items = np.concatenate([b[1] for b in blocks]) if blocks else np.empty(0, dtype=np.int64)
    order = np.argsort(users, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(per_user_counts)]).astype(np.int64)
    return ptr, items[order]


def candidate_csr_device(matchers, num_users: int, device):
    """candidate_csr with every stage on the device: (ptr int32[U + 1], idx int32[]) tensors, or None when a matcher
    has no device form.  Row u = cat(m.get_matches(u) for m in matchers), -1 pads dropped, order kept."""
    if not matchers or not all(hasattr(m, "matches_for_all_device") for m in matchers):
        return None
    cat = t.cat([m.matches_for_all_device(num_users, device) for m in matchers], dim=1)
    keep = cat >= 0
    ptr = t.zeros(num_users + 1, dtype=t.int64, device=device)
    t.cumsum(keep.sum(dim=1), dim=0, out=ptr[1:])
    return ptr.to(t.int32), cat[keep].to(t.int32)


class DeviceGraphSampler:
    def __init__(self, config, graph: HeteroData, users_adj_list, articles_adj_list, batch_size: Optional[int] = None,
                 randomization: bool = True, device: str = "cuda", seed: int = 0, prefetch: bool = True,
                 train: bool = True, matchers=None, shuffle: bool = True, emit_csr: bool = True):
        """emit_csr: also write each batch's edges as the two sorted CSRs the encoder consumes (mi_sampler_emit_csr),
        attached to edge_index as `_sorted_csr`; the encoder then builds no CSR of its own for the batch.
        train=False: evaluation samples as GraphDataset(train=False) builds them — the label-0 edges are the
        matchers' candidates (minus purchases, plus purchases no matcher proposed; data/dataset.py:94-105)."""
        self.config, self.device, self.seed = config, t.device(device), int(seed)
        self.prefetch, self._side = ("thread" if prefetch == "thread" else bool(prefetch)), None
        self.train, self.shuffle = bool(train), bool(shuffle)
        self.emit_csr = bool(emit_csr) and int(config.n_hop_neighbors) * int(config.num_neighbors) <= 512
        self.batch_size = int(batch_size if batch_size is not None else config.batch_size)
        self.randomization = randomization
        ux, ax = graph[Constants.node_user].x, graph[Constants.node_item].x
        n_users, n_articles = ux.shape[0], ax.shape[0]
        users, articles = AdjList(users_adj_list, n_users), AdjList(articles_adj_list, n_articles)
        ei = graph[Constants.edge_key].edge_index
        self.num_edges, self.id_max = int(ei.shape[1]), int(ei[1].max())
        dev = self.device
        to32 = lambda a: t.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
        self.uptr, self.uidx = to32(users.ptr), to32(users.idx)
        self.aptr, self.aidx = to32(articles.ptr), to32(articles.idx)
        self.user_x, self.article_x = ux.to(dev), ax.to(dev)
        self.num_users, self.num_articles = n_users, n_articles
        max_deg = int(np.diff(users.ptr).max()) if n_users else 1
        self.max_pos = max(2, math.floor(max_deg * config.positive_edges_ratio) if randomization else 2)
        self.max_neg = max(1, config.k - 1, int(config.negative_edges_ratio * self.max_pos))
        self.cptr = self.cidx = None
        if not self.train:
            assert matchers is not None, "Must provide matchers for test"
            on_dev = candidate_csr_device(matchers, n_users, dev) if dev.type == "cuda" else None
            if on_dev is not None:  # N3: proposals computed and kept on the device
                self.cptr, self.cidx = on_dev
                widest = int((self.cptr[1:] - self.cptr[:-1]).max()) if n_users else 0
                if self.cidx.numel() == 0:
                    self.cidx = t.zeros(1, dtype=t.int32, device=dev)
            else:
                cptr, cidx = candidate_csr(matchers, n_users)
                self.cptr, self.cidx = to32(cptr), to32(cidx if cidx.size else np.zeros(1, dtype=np.int64))
                widest = int(np.diff(cptr).max())
            self.max_neg = max(self.max_neg, widest + max_deg)
        self._desc = self._make_desc(self.batch_size)
        self._ws = t.empty(int(_lib.lib().mi_sampler_workspace_bytes(ctypes.byref(self._desc))), dtype=t.uint8, device=dev)
        self.step = 0
        # Config.other_edge_types: attribute node types (article, name, T), data/relations.py.  The CSRs and graph[T].x go to
        # the device once; none (the default) leaves every path below as it was.
        self._rels = resolve_relations(config, graph)
        self._rel_arr, self._rel_ws, self._rel_dev, self._pinned_serial = None, None, [], None
        if self._rels:
            if len(self._rels) > _lib.MI_SAMPLER_MAX_RELATIONS:
                raise ValueError(f"other_edge_types: {len(self._rels)} relations, the device sampler takes "
                                 f"{_lib.MI_SAMPLER_MAX_RELATIONS}")
            self._rel_arr = (SamplerRelation * len(self._rels))()
            for i, r in enumerate(self._rels):
                ptr, idx = to32(r.ptr), to32(r.idx if r.idx.size else np.zeros(1, dtype=np.int64))
                self._rel_dev.append((ptr, idx, r.x.to(dev)))
                self._rel_arr[i] = SamplerRelation(ptr.data_ptr(), idx.data_ptr(), r.n_targets)
            n_ws = int(_lib.lib().mi_sampler_relations_workspace_bytes(ctypes.byref(self._desc), self._rel_arr, len(self._rels)))
            if n_ws == 0:
                raise _lib.MiError("mi_sampler_relations_workspace_bytes declined the relations")
            self._rel_ws = t.empty(n_ws, dtype=t.uint8, device=dev)

    def _make_desc(self, batch: int) -> SamplerDesc:
        c = self.config
        return SamplerDesc(batch, int(c.n_hop_neighbors), int(c.num_neighbors), int(c.k), 1 if self.randomization else 0,
                           self.max_pos, self.max_neg, 0, self.num_users, self.num_articles, self.num_edges, self.id_max,
                           self.uptr.data_ptr(), self.uidx.data_ptr(), self.aptr.data_ptr(), self.aidx.data_ptr(),
                           float(c.positive_edges_ratio), float(c.negative_edges_ratio),
                           int(getattr(c, "reject_min_entries", 0) or 0),
                           self.cptr.data_ptr() if self.cptr is not None else None,
                           self.cidx.data_ptr() if self.cidx is not None else None)

    def __len__(self) -> int:
        return (self.num_users + self.batch_size - 1) // self.batch_size

    def sample(self, seed_users: Tensor, step: Optional[int] = None, raw: bool = False):
        """Collated batch for `seed_users` (int64, any device). raw=True returns the flat arrays."""
        if step is None:
            step = self.step
            self.step += 1
        seeds = seed_users.to(self.device, t.int64).contiguous()
        B = seeds.numel()
        if B > self.batch_size:
            raise ValueError("more seed users than the sampler's batch size")
        desc = self._desc if B == self.batch_size else self._make_desc(B)
        L = _lib.lib()
        stream = _lib.current_stream()
        if self._rels:  # walk and relation counts enqueued together, ONE wait for all the totals
            if self._pinned_serial is None:
                self._pinned_serial = t.empty(4 + 2 * len(self._rels), dtype=t.int32).pin_memory()
            pinned = self._pinned_serial
            check(L.mi_sampler_count_async(ctypes.byref(desc), seeds.data_ptr(), self.seed & (2**64 - 1), int(step) & (2**64 - 1),
                                           self._ws.data_ptr(), self._ws.numel(), pinned.data_ptr(), stream), "mi_sampler_count_async")
            self._count_relations(desc, self._ws, self._rel_ws, pinned, stream)
            t.cuda.current_stream(self.device).synchronize()
            got = pinned.tolist()
            return self._emit(seeds, desc, got[:4], stream, raw, rel_totals=got[4:])
        totals = (ctypes.c_int64 * 4)()
        check(L.mi_sampler_count(ctypes.byref(desc), seeds.data_ptr(), self.seed & (2**64 - 1), int(step) & (2**64 - 1),
                                 self._ws.data_ptr(), self._ws.numel(), totals, stream), "mi_sampler_count")
        return self._emit(seeds, desc, [int(x) for x in totals], stream, raw)

    def _count_relations(self, desc: SamplerDesc, ws: Tensor, rel_ws: Tensor, pinned: Tensor, stream: int) -> None:
        """Right behind phase A on `stream`: the relations' {T nodes, edges} totals land in pinned[4:]."""
        check(_lib.lib().mi_sampler_count_relations_async(ctypes.byref(desc), self._rel_arr, len(self._rels), ws.data_ptr(),
                                                          ws.numel(), rel_ws.data_ptr(), rel_ws.numel(),
                                                          pinned.data_ptr() + 16, stream), "mi_sampler_count_relations_async")

    def _emit_relations(self, desc: SamplerDesc, totals, rel_totals, stream: int, ws: Tensor, rel_ws: Tensor):
        """Phase B of the relations: ([per relation: T_ids, T_ptr, edge3, (by article, by T) CSRs], storages)."""
        from .. import ops
        n_rel, na, B, dev = len(self._rels), int(totals[1]), int(desc.batch), self.device
        if any(int(x) < 0 for x in rel_totals):
            raise _lib.MiError("other_edge_types: a batch's relation edges do not fit int32")
        r4 = lambda n: (n + 3) & ~3
        s64, s32 = [], []
        for i in range(n_rel):
            nt, ne = int(rel_totals[2 * i]), int(rel_totals[2 * i + 1])
            s64 += [r4(nt), r4(B + 1), r4(3 * ne)]
            s32 += [r4(na + 1), r4(ne), r4(nt + 1), r4(ne), r4(max(nt, 1))]
        b64, b32 = t.empty(sum(s64), dtype=t.int64, device=dev), t.empty(sum(s32), dtype=t.int32, device=dev)
        outs = (SamplerRelationOut * n_rel)()
        res, o64, o32 = [], 0, 0
        for i in range(n_rel):
            nt, ne = int(rel_totals[2 * i]), int(rel_totals[2 * i + 1])
            p64, p32 = [], []
            for n_alloc in s64[3 * i:3 * i + 3]:
                p64.append(o64)
                o64 += n_alloc
            for n_alloc in s32[5 * i:5 * i + 5]:
                p32.append(o32)
                o32 += n_alloc
            t_ids, t_ptr = b64[p64[0]:p64[0] + nt], b64[p64[1]:p64[1] + B + 1]
            edge3 = b64[p64[2]:p64[2] + 3 * ne].view(3, ne)
            a_rowptr, a_col = b32[p32[0]:p32[0] + na + 1], b32[p32[1]:p32[1] + ne]
            t_rowptr, t_col, t_cur = b32[p32[2]:p32[2] + nt + 1], b32[p32[3]:p32[3] + ne], b32[p32[4]:p32[4] + max(nt, 1)]
            outs[i] = SamplerRelationOut(t_ids.data_ptr() if nt else None, t_ptr.data_ptr(), edge3.data_ptr() if ne else None,
                                         a_rowptr.data_ptr(), a_col.data_ptr() if ne else None, t_rowptr.data_ptr(),
                                         t_col.data_ptr() if ne else None, t_cur.data_ptr())
            csr = (ops.DeviceCSR(na, nt, a_rowptr, a_col), ops.DeviceCSR(nt, na, t_rowptr, t_col))
            res.append((t_ids, t_ptr, edge3, csr))
        tot = (ctypes.c_int64 * 4)(*[int(x) for x in totals])
        rtot = (ctypes.c_int64 * (2 * n_rel))(*[int(x) for x in rel_totals])
        check(_lib.lib().mi_sampler_emit_relations(ctypes.byref(desc), self._rel_arr, n_rel, ws.data_ptr(), ws.numel(), tot,
                                                   rel_ws.data_ptr(), rel_ws.numel(), rtot, outs, stream),
              "mi_sampler_emit_relations")
        return res, [b64, b32]

    def _emit(self, seeds: Tensor, desc: SamplerDesc, totals, stream: int, raw: bool = False, ws: Optional[Tensor] = None,
              rel_totals=None, rel_ws: Optional[Tensor] = None):
        """Phase B on `stream` (the current torch stream must be that stream: the feature gathers follow it).  ws: the
        workspace phase A of this batch ran in (default: the sampler's own); rel_totals / rel_ws: the same for the relations."""
        ws = self._ws if ws is None else ws
        nu, na, ne, nl = totals
        B = seeds.numel()
        L = _lib.lib()
        tot = (ctypes.c_int64 * 4)(nu, na, ne, nl)
        dev = self.device
        # ONE int64 block and ONE int32 block per batch, the outputs are views of them (round 4: 18 allocations per batch and
        # 14 record_stream calls were a visible part of a host-bound loop).  edge_index / edge_label_index are written as
        # [3, n] — row 2 repeats row 0 — so the reversed relation's index (data/dataset.py: flip(0)) is rows 1..2 of the same
        # buffer: a view, not two flip launches.
        r4 = lambda n: (n + 3) & ~3                      # every piece starts on a 32-byte (int64) / 16-byte (int32) boundary
        sizes = (r4(nu), r4(na), r4(3 * ne), r4(3 * nl), r4(nl), r4(B + 1), r4(B + 1))
        blk = t.empty(sum(sizes), dtype=t.int64, device=dev)
        off, parts = 0, []
        for n_alloc in sizes:
            parts.append(off)
            off += n_alloc
        user_ids, article_ids = blk[parts[0]:parts[0] + nu], blk[parts[1]:parts[1] + na]
        edge3 = blk[parts[2]:parts[2] + 3 * ne].view(3, ne)
        label3 = blk[parts[3]:parts[3] + 3 * nl].view(3, nl)
        labels = blk[parts[4]:parts[4] + nl]
        user_ptr, article_ptr = blk[parts[5]:parts[5] + B + 1], blk[parts[6]:parts[6] + B + 1]
        edge_index, label_index = edge3[0:2], label3[0:2]
        check(L.mi_sampler_emit3(ctypes.byref(desc), seeds.data_ptr(), ws.data_ptr(), ws.numel(), tot,
                                 user_ids.data_ptr(), article_ids.data_ptr(), edge3.data_ptr() if ne else None,
                                 label3.data_ptr(), labels.data_ptr(), user_ptr.data_ptr(), article_ptr.data_ptr(), 1,
                                 stream), "mi_sampler_emit3")
        csr = None
        blocks = [blk]
        if getattr(self, "emit_csr", False):
            from .. import ops
            s32 = (r4(nu + 1), r4(na + 1), r4(ne), r4(ne), r4(max(na, 1)))
            b32 = t.empty(sum(s32), dtype=t.int32, device=dev)
            o0, o1, o2, o3 = s32[0], s32[0] + s32[1], s32[0] + s32[1] + s32[2], s32[0] + s32[1] + s32[2] + s32[3]
            u_rowptr, a_rowptr = b32[0:nu + 1], b32[o0:o0 + na + 1]
            u_col, a_col, cursor = b32[o1:o1 + ne], b32[o2:o2 + ne], b32[o3:o3 + max(na, 1)]
            check(L.mi_sampler_emit_csr(ctypes.byref(desc), ws.data_ptr(), ws.numel(), tot, u_rowptr.data_ptr(),
                                        u_col.data_ptr() if ne else None, a_rowptr.data_ptr(), a_col.data_ptr() if ne else None,
                                        cursor.data_ptr(), stream), "mi_sampler_emit_csr")
            # (rows = customers, rows = articles): by-source and by-destination forms of the customer -> article relation
            csr = (ops.DeviceCSR(nu, na, u_rowptr, u_col), ops.DeviceCSR(na, nu, a_rowptr, a_col))
            blocks.append(b32)
        rels = None
        if self._rels:
            rels, rel_blocks = self._emit_relations(desc, totals, rel_totals, stream, ws, self._rel_ws if rel_ws is None else rel_ws)
            blocks += rel_blocks
        if raw:
            out = {"user_ids": user_ids, "article_ids": article_ids, "edge_index": edge_index,
                    "edge_label_index": label_index, "edge_label": labels, "user_ptr": user_ptr, "article_ptr": article_ptr}
            if csr is not None:
                out["csr_by_customer"], out["csr_by_article"] = csr
            if rels is not None:
                out["relations"] = {r.key: {"T_ids": ids, "T_ptr": ptr, "edge_index": e3[0:2], "edge3": e3,
                                            "csr_by_article": c[0], "csr_by_target": c[1]}
                                    for r, (ids, ptr, e3, c) in zip(self._rels, rels)}
            return out
        data = HeteroData()
        xc, xa = self.user_x[user_ids], self.article_x[article_ids]
        data[Constants.node_user].x = xc
        data[Constants.node_item].x = xa
        data[Constants.node_user].n_id = user_ids
        data[Constants.node_item].n_id = article_ids
        if csr is not None:
            edge_index._sorted_csr = csr  # (by source, by destination), read by model/layers.py BipartiteGraph.of
        data[Constants.edge_key].edge_index = edge_index
        data[Constants.edge_key].edge_label_index = label_index
        data[Constants.edge_key].edge_label = labels
        rev = edge3[1:3]                  # = edge_index.flip(0): rows (article, customer)
        rev._reverse_of = edge_index      # lets the encoder reuse the forward relation's sorted CSRs (model/layers.py)
        data[Constants.rev_edge_key].edge_index = rev
        data[Constants.rev_edge_key].edge_label_index = label3[1:3]
        data[Constants.rev_edge_key].edge_label = labels
        extra_x = []
        if rels is not None:   # no edge_label* on these stores (data/dataset_neo.py:85-91)
            for r, (_, _, x_all), (ids, ptr, e3, c) in zip(self._rels, self._rel_dev, rels):
                xt = x_all[ids]
                data[r.target].x = xt
                data[r.target].n_id = ids
                data[r.target].ptr = ptr
                fwd, rev = e3[0:2], e3[1:3]
                fwd._sorted_csr = c       # (by article, by T)
                rev._reverse_of = fwd
                data[r.key].edge_index = fwd
                data[r.rev_key].edge_index = rev
                extra_x.append(xt)
        data._blocks = blocks + [xc, xa] + extra_x  # the storages behind every tensor of the batch (the iterator's record_stream calls)
        data._seed_users, data._user_ptr = seeds, user_ptr   # per-sample structure (run_submission.make_predictions' sync-free path)
        data._article_ptr = article_ptr                       # with data[T].ptr: which articles / attribute nodes belong to which sample
        data._max_candidates = int(self.max_neg)             # capacity of a sample's label-0 list
        return data

    def iter_users(self, users: Tensor) -> Iterator[HeteroData]:
        """The batches of `users` (int64, in this order, batch_size at a time) through the same pipelined iterator as an epoch:
        batch i is sampled with Philox step self.step + i, exactly what sample(users[i * B:(i + 1) * B], step=self.step + i)
        returns — evaluation of a subset of the customers (a submission shard, held-out users) without a host wait per batch.
        The order belongs to the iterator returned HERE, whichever iterator of this sampler is advanced first.  Ids outside
        [0, num_users) raise IndexError before anything is uploaded: the walk kernels index with them unchecked."""
        order = users.detach().to("cpu", t.int64).contiguous().view(-1)
        if order.numel() and (int(order.min()) < 0 or int(order.max()) >= self.num_users):
            bad = order[(order < 0) | (order >= self.num_users)]
            raise IndexError(f"iter_users: {int(bad.numel())} user id(s) outside [0, {self.num_users}), e.g. {int(bad[0])}")
        return self._epoch(order)

    def __iter__(self) -> Iterator[HeteroData]:
        """One epoch: every user once, shuffled (DataLoader(shuffle=True) semantics).  With `prefetch` (default)
        sampling runs three batches ahead on a side stream while the consumer trains on batch i: nothing of the
        sampler sits between two steps.  Same batches, same order, same Philox steps as the serial loop.
        An iterator abandoned mid-epoch (break, close(), dropped) orders the consumer's stream after whatever it had
        queued on the side stream; self.step counts the batches handed out."""
        return self._epoch(None)

    def _epoch(self, order: Optional[Tensor]) -> Iterator[HeteroData]:
        if order is None:
            g = t.Generator(device="cpu").manual_seed(self.seed + self.step)
            order = t.randperm(self.num_users, generator=g) if self.shuffle else t.arange(self.num_users)
        n_order = int(order.numel())
        batches = [order[b:b + self.batch_size] for b in range(0, n_order, self.batch_size)]
        if not getattr(self, "prefetch", True) or not batches:
            for seeds in batches:
                yield self.sample(seeds)
            return
        L = _lib.lib()
        main = t.cuda.current_stream(self.device)
        DEPTH = 3   # batches in flight: the walk of batch i + 3 is enqueued while the consumer trains on batch i (see below)
        if getattr(self, "_side", None) is None:
            self._side = t.cuda.Stream(device=self.device)
            self._pinned = [t.empty(4 + 2 * len(self._rels), dtype=t.int32).pin_memory() for _ in range(DEPTH)]
            # a workspace per batch in flight: phase A of batch j + DEPTH may be enqueued before phase B of batch j + 1 ...
            self._ws_ring = [self._ws] + [t.empty_like(self._ws) for _ in range(DEPTH - 1)]
            self._rel_ws_ring = [self._rel_ws] + [t.empty_like(self._rel_ws) for _ in range(DEPTH - 1)] if self._rels else None
        side = self._side
        step0 = self.step

        # the epoch's seed order goes to the device ONCE (round 4: a 24-element host-to-device copy per batch was 40 us of the
        # loop's host time — the loop is host-bound, tools/prof_host_native.py); a batch's seeds are a view of it
        order_dev = order.to(self.device, t.int64)
        order_dev.record_stream(side)   # read by the side stream's walks: its memory is not reused before they are done
        batches_dev = [order_dev[b:b + self.batch_size] for b in range(0, n_order, self.batch_size)]

        side_raw = side.cuda_stream

        def start(i: int):  # phase A of batch i, enqueued on the side stream (raw handle: no torch op, no stream context), no host wait
            seeds = batches_dev[i]
            desc = self._desc if seeds.numel() == self.batch_size else self._make_desc(seeds.numel())
            check(L.mi_sampler_count_async(ctypes.byref(desc), seeds.data_ptr(), self.seed & (2**64 - 1),
                                           int(step0 + i) & (2**64 - 1), self._ws_ring[i % DEPTH].data_ptr(), self._ws_ring[i % DEPTH].numel(),
                                           self._pinned[i % DEPTH].data_ptr(), side_raw), "mi_sampler_count_async")
            if self._rels:  # behind the walk, before the event: the same wait covers both sets of totals
                self._count_relations(desc, self._ws_ring[i % DEPTH], self._rel_ws_ring[i % DEPTH], self._pinned[i % DEPTH], side_raw)
            ev = t.cuda.Event()
            ev.record(side)
            return seeds, desc, ev

        def finish(i: int, pend):  # phase B of batch i on the side stream, once its four totals have landed
            seeds, desc, ev = pend
            ev.synchronize()
            totals = self._pinned[i % DEPTH].tolist()
            with t.cuda.stream(side):
                if self._rels:
                    data = self._emit(seeds, desc, totals[:4], side_raw, ws=self._ws_ring[i % DEPTH], rel_totals=totals[4:],
                                      rel_ws=self._rel_ws_ring[i % DEPTH])
                else:
                    data = self._emit(seeds, desc, totals, side_raw, ws=self._ws_ring[i % DEPTH])
                ready = t.cuda.Event()
                ready.record(side)
            return data, ready

        def hand_out(data, ready):
            main.wait_event(ready)
            for blk in data._blocks:      # every tensor of the batch is a view of one of these storages
                blk.record_stream(main)
            return data

        # THREE batches ahead (round 4; two before): while the consumer trains on batch i, batch i+1 is being emitted and the
        # walks of batches i+2 and i+3 are queued behind it.  With two, finish(i+2) waited for a walk that had been enqueued
        # only one host-side step issue (~0.2 ms) earlier — the walk + emit chain of a batch is ~0.3 ms of side-stream kernels
        # plus ~0.15 ms of host work, and the loop ran at THAT period (0.47 ms) although the step's kernels take 0.41 and the
        # host issues an iteration in ~0.3 (tools/prof_host_native.py).  Now the wait is on work enqueued a whole iteration
        # earlier.  Side-stream order: ... emit(i+1), count(i+3), emit(i+2), count(i+4) ...; batch j works in workspace j mod 3,
        # so count(j+3) overwrites workspace j mod 3 only after emit(j) — same stream, enqueued earlier.
        side.wait_stream(main)
        nb = len(batches)
        if getattr(self, "prefetch", True) == "thread":
            # the sampler's host side (a dozen launches and allocations per batch) on a thread of its own: the training
            # step is bound by its own launches, so this takes the sampler's share off the loop's critical path
            import queue
            import threading
            out: "queue.Queue" = queue.Queue(maxsize=2)
            dev_index = self.device.index if self.device.index is not None else t.cuda.current_device()
            stop = threading.Event()

            def produce():
                try:
                    t.cuda.set_device(dev_index)
                    pend = start(0)
                    for i in range(nb):
                        item = finish(i, pend)
                        pend = start(i + 1) if i + 1 < nb else None
                        while not stop.is_set():
                            try:
                                out.put(item, timeout=0.05)
                                break
                            except queue.Full:
                                continue
                        if stop.is_set():
                            return
                except BaseException as exc:  # surfaces in the consumer
                    out.put(exc)

            import sys
            interval = sys.getswitchinterval()
            sys.setswitchinterval(min(interval, float(os.environ.get("LAPLACE_SAMPLER_SWITCH", "1e-4"))))  # neither thread may sit on the interpreter lock for 5 ms
            worker = threading.Thread(target=produce, name="laplace-sampler", daemon=True)
            worker.start()
            try:
                for i in range(nb):
                    item = out.get()
                    if isinstance(item, BaseException):
                        raise item
                    self.step = step0 + i + 1
                    yield hand_out(*item)
            finally:
                stop.set()
                worker.join()
                sys.setswitchinterval(interval)
                t.cuda.current_stream(self.device).wait_stream(side)
            return
        try:
            pend = {j: start(j) for j in range(min(DEPTH, nb))}      # phase A of the first DEPTH batches
            cur = finish(0, pend.pop(0))
            for i in range(nb):
                data, ready = cur
                if i + 1 < nb:
                    cur = finish(i + 1, pend.pop(i + 1))
                    if i + DEPTH < nb:
                        pend[i + DEPTH] = start(i + DEPTH)
                self.step = step0 + i + 1
                yield hand_out(data, ready)
        finally:   # an abandoned epoch leaves up to DEPTH walks and an emit queued: the consumer's stream goes after them
            t.cuda.current_stream(self.device).wait_stream(side)
