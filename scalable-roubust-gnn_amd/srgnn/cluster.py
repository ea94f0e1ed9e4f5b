"""Cluster-GCN mini-batches on the device: the sub-graph induced by a node set, and the loader around it.

The reference's second training function, train_minibatch, partitions the graph with PyG's
ClusterData(data, num_parts) and trains every step on the sub-graph induced by the union of batch_size of the
parts (ClusterLoader).  This module is that path for a DeviceCSR:

  induced_subgraph(A, nodes)   rows `nodes` of A, filtered to the columns in `nodes` and relabelled: scipy's
                               A[S][:, S], built by srg_csr_induced_f32 (count, prefix sum, fill); with
                               relabel=False the row slice A[S]
  ClusterData(A, P, part)      a partition of the nodes: partptr and perm, the graph itself is not permuted
  ClusterLoader(cd, batch)     per epoch a host-side shuffle of the parts; each item is a ClusterBatch with the
                               batch's node ids, its DeviceCSR and the layers' operators built from it

METIS and PyG are absent here: ClusterData takes the assignment `part` from the caller (from METIS or anything
else) and otherwise cuts the rows into contiguous blocks; what the loader yields is restated from PyG's
published description (the batch's nodes are its parts' nodes, part after part, and its edges those with both
ends in the batch), and parity with PyG's bits is not pinned.  The batch operator's values are the full
operator's, restricted: Â is not renormalised on the sub-graph.  There is no torch fallback: the extraction is
a kernel of libsrgnn_hip.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .csr import DeviceCSR, _dev
from .graph_conv import batch_rows

__all__ = ["induced_subgraph", "ClusterData", "ClusterLoader", "ClusterBatch"]


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def induced_subgraph(A: DeviceCSR, nodes, relabel: bool = True, eid: bool = False):
    """(sub, ids[, eid]): row b of `sub` is row ids[b] of A.

    nodes: a tensor, list, ndarray or range of row ids (graph_conv.batch_rows: negative ids wrap, an id out of
    range raises IndexError, bool or float ids TypeError, a shape that is not 1-D ValueError, all before any
    launch); a node set is a set, so a repeated id raises ValueError.  ids: the wrapped ids, int64 [B] on A's device.
    relabel=True (a square A): the entries whose column is in the set, stored with column id b where
    ids[b] is the column; sub is [B, B] and equals scipy's A[S][:, S].  relabel=False: every entry with its
    column id as stored; sub is [B, n_cols] and equals scipy's A[S].  Entries keep the stored order, duplicates
    stay, values are copied bit for bit.  eid=True also returns int64 [nnz(sub)]: entry t of sub is entry
    eid[t] of A, for edge attributes or a permutation carried across.

    Two launches of srg_csr_induced_f32 with torch.cumsum between them.  The one host read of ptr[-1], which
    sizes the outputs, is the only synchronisation; the temporaries are cnt [B], ptr [B + 1] and pos [n]."""
    if not isinstance(A, DeviceCSR):
        raise TypeError("induced_subgraph takes a DeviceCSR")
    if A.is_span or A.schedules_subset:
        raise ValueError("induced_subgraph takes a whole operator, not a column block or row group")
    if relabel and A.n_rows != A.n_cols:
        raise ValueError(f"relabel=True takes a square operator, got {A.n_rows}x{A.n_cols}")
    ids, pos, unique = batch_rows(nodes, A.n_rows, A.device)
    if not unique:
        raise ValueError("nodes repeats an id: a node set holds every node once")
    dev = _dev(A.device)
    B = ids.numel()
    cnt = torch.empty(B, dtype=torch.int64, device=dev)
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    args = (A.indptr.data_ptr(), _ptr(A.indices), _ptr(A.values), A.n_rows, A.n_cols, _ptr(ids), B,
            _ptr(pos) if relabel else None)
    _lib.call(dev, "srg_csr_induced_f32", 0, *args, _ptr(cnt), None, None, None, None, _lib.stream(dev))
    if B:
        torch.cumsum(cnt, 0, out=ptr[1:])
    nnz = int(ptr[-1]) if B else 0
    out_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(nnz, dtype=torch.float32, device=dev)
    out_eid = torch.empty(nnz, dtype=torch.int64, device=dev) if eid else None
    if nnz:
        _lib.call(dev, "srg_csr_induced_f32", 1, *args, None, ptr.data_ptr(), out_idx.data_ptr(),
                  out_val.data_ptr(), _ptr(out_eid), _lib.stream(dev))
    sub = DeviceCSR(ptr, out_idx, out_val, B, B if relabel else A.n_cols, None, None, None, None,
                    thresholds=A.thresholds)
    return (sub, ids, out_eid) if eid else (sub, ids)


def _default_part(indptr: torch.Tensor, num_parts: int) -> torch.Tensor:
    """Contiguous row blocks of near-equal rows + entries: the multi-GPU row partition's balancer
    (dist.balanced_row_starts) over the weights 1 + row length."""
    from .dist import balanced_row_starts
    ip = indptr.to(torch.int64).cpu()
    n = ip.numel() - 1
    starts = torch.tensor(balanced_row_starts(ip + torch.arange(n + 1, dtype=torch.int64), num_parts), dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(num_parts, dtype=torch.int64), starts[1:] - starts[:-1])


class ClusterData:
    """A partition of an operator's nodes into num_parts parts, as PyG's ClusterData holds one.

    A: a square DeviceCSR, or a scipy sparse matrix (moved to `device`), over targets as adj_t is.
    part: an integer [n] assignment with values in [0, num_parts) (checked; parts may be empty), on any
    device; None cuts the rows into contiguous blocks of near-equal rows + entries (partition quality is not
    this module's business: pass METIS's assignment for Cluster-GCN's).
    partptr int64 [P + 1] and perm int64 [n] (the node ids sorted stably by part) are built with torch ops
    on part's device; part p's nodes are perm[partptr[p]:partptr[p + 1]], in increasing id.  The graph itself
    is not permuted: batches are extracted from A in original ids."""

    def __init__(self, A, num_parts: int, part=None, device=None):
        num_parts = int(num_parts)
        if num_parts < 1:
            raise ValueError(f"num_parts={num_parts} < 1")
        if not isinstance(A, DeviceCSR):
            import scipy.sparse as sp
            if not sp.issparse(A):
                raise TypeError(f"ClusterData takes a DeviceCSR or a scipy sparse matrix, got {type(A).__name__}")
            if A.shape[0] != A.shape[1]:
                raise ValueError(f"ClusterData takes a square operator, got {A.shape}")
            A = DeviceCSR.from_scipy(A.tocsr(), device=device)
        if A.n_rows != A.n_cols:
            raise ValueError(f"ClusterData takes a square operator, got {A.n_rows}x{A.n_cols}")
        n = A.n_rows
        if part is None:
            part = _default_part(A.indptr, num_parts)
        else:
            part = torch.as_tensor(part)
            if part.dtype == torch.bool or part.is_floating_point() or part.is_complex():
                raise TypeError(f"part must hold integer part ids, got {part.dtype}")
            if part.dim() != 1 or part.numel() != n:
                raise ValueError(f"part must be a 1-D assignment of {n} nodes, got shape {tuple(part.shape)}")
            part = part.to(torch.int64)
            if n and (int(part.min()) < 0 or int(part.max()) >= num_parts):
                raise ValueError(f"a part id is outside [0, {num_parts})")
        self.A, self.num_parts, self.part = A, num_parts, part
        self.perm = torch.sort(part, stable=True).indices
        self.partptr = torch.zeros(num_parts + 1, dtype=torch.int64, device=part.device)
        if n:
            torch.cumsum(torch.bincount(part, minlength=num_parts), 0, out=self.partptr[1:])

    def __len__(self):
        return self.num_parts

    def nodes_of(self, parts) -> torch.Tensor:
        """The node ids of `parts` (a sequence of part ids), part after part in the order given."""
        bounds = self.partptr.tolist()
        pieces = [self.perm[bounds[p]:bounds[p + 1]] for p in parts]
        return torch.cat(pieces) if pieces else self.perm[:0]


class ClusterBatch:
    """One mini-batch: nodes (int64 [B], original ids, on the operator's device), csr (the induced DeviceCSR,
    [B, B], relabelled to positions in `nodes`), parts (the part ids it was made of), and the layers'
    operators, each built on first use by the class that owns it."""

    def __init__(self, A: DeviceCSR, parts, nodes):
        self.parts = list(parts)
        self._A, self._eid = A, None
        self.csr, self.nodes = induced_subgraph(A, nodes, relabel=True)

    @property
    def eid(self) -> torch.Tensor:
        """int64 [nnz(csr)]: entry t of csr is entry eid[t] of the full operator.  Built when first asked for,
        by a second extraction that also writes the entry ids (training on Â alone never needs them)."""
        if self._eid is None:
            self._eid = induced_subgraph(self._A, self.nodes, relabel=True, eid=True)[2]
        return self._eid

    def graph_conv_operator(self):
        """GraphConvOperator.from_device_csr(csr): the restricted values, not renormalised, and the transpose
        that class builds."""
        from .graph_conv import GraphConvOperator
        return GraphConvOperator.from_device_csr(self.csr)

    def gat_graph(self, add_self_loops: bool = True):
        """GATGraph.from_device_csr(csr, add_self_loops)."""
        from .gat import GATGraph
        return GATGraph.from_device_csr(self.csr, add_self_loops)

    def __repr__(self):
        return f"ClusterBatch(parts={self.parts}, nodes={self.nodes.numel()}, nnz={self.csr.indices.numel()})"


class ClusterLoader:
    """Iterates over a ClusterData in batches of batch_size parts, as PyG's ClusterLoader does: len is
    ceil(P / batch_size), an epoch visits every part exactly once (the last batch may be short), and with
    shuffle the parts' order is torch.randperm(P, generator=generator) on the host, drawn anew per epoch.
    Each item is a ClusterBatch of the sub-graph induced by the batch's parts."""

    def __init__(self, cluster_data: ClusterData, batch_size: int, shuffle: bool = True, generator=None):
        if not isinstance(cluster_data, ClusterData):
            raise TypeError("ClusterLoader takes a ClusterData")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} < 1")
        self.cluster_data, self.batch_size, self.shuffle, self.generator = cluster_data, batch_size, bool(shuffle), generator

    def __len__(self):
        return math.ceil(self.cluster_data.num_parts / self.batch_size)

    def part_batches(self):
        """The epoch's batches as lists of part ids (draws the epoch's permutation)."""
        P = self.cluster_data.num_parts
        order = torch.randperm(P, generator=self.generator).tolist() if self.shuffle else list(range(P))
        return [order[i:i + self.batch_size] for i in range(0, P, self.batch_size)]

    def __iter__(self):
        cd = self.cluster_data
        for parts in self.part_batches():
            yield ClusterBatch(cd.A, parts, cd.nodes_of(parts))
